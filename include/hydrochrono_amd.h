/* hydrochrono_amd.h -- C ABI of the MI355X-native HydroChrono hydro-force path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types.  Each entry point names
 * the reference interface (file:line relative to the HydroChrono tree @2025-10-31) it replaces.
 * INTEGRATION.md shows the Chrono-side binding (ChFunction / ChLoadCustomMultiple subclasses) that
 * forwards to these calls; the headers under include/hydroc_amd are that binding.
 *
 * Conventions
 *   N   = number of hydro bodies of the whole system, D = 6N degrees of freedom.
 *   A context may own only the output rows of bodies [body_begin, body_end) (multi-GPU row sharding,
 *   SURVEY 8e); n_local = body_end - body_begin, D_local = 6*n_local.  Per-step INPUTS are always
 *   the full N-body state, per-step OUTPUTS have D_local entries.
 *   All arrays are IEEE double, row-major ("file order" of the BEMIO HDF5 datasets) unless stated.
 *   Every function returns an hc_status; hc_last_error() holds the message of the last failure.
 *   One host thread drives a context (same contract as TestHydro: its per-time cache is
 *   unsynchronised, src/hydro_forces.cpp:742-748).
 *   The library computes on the GPU only.  There is no CPU fallback: hc_create fails with
 *   HC_ERR_DEVICE when no gfx950 device is usable.
 */
#ifndef HYDROCHRONO_AMD_H
#define HYDROCHRONO_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hc_ctx hc_ctx;

typedef enum hc_status {
    HC_OK               = 0,
    HC_ERR_RUNTIME      = 1, /* the reference throws std::runtime_error here */
    HC_ERR_OUT_OF_RANGE = 2, /* the reference throws std::out_of_range here  */
    HC_ERR_INVALID      = 3, /* bad argument / call order                     */
    HC_ERR_DEVICE       = 4, /* HIP runtime failure or no usable GPU         */
    HC_ERR_UNSUPPORTED  = 5  /* optional component not built (e.g. HDF5)      */
} hc_status;

/* ------------------------------------------------------------------------------------------------
 * Lifecycle.  Replaces TestHydro::TestHydro / ~TestHydro (src/hydro_forces.cpp:170-242).
 * ---------------------------------------------------------------------------------------------- */
const char* hc_version(void);
int hc_device_count(void); /* number of visible HIP devices; does not initialise a context */
/* Where the host thread that steps should run.  A synchronous step is a round trip between one host thread and one GPU: a doorbell
 * store into the GPU's MMIO page, stores through its BAR, and a spin on pinned memory the GPU writes.  From a core of the OTHER
 * socket every one of them crosses the socket interconnect: 64 bodies 11.5-11.8 us per hc_step against 10.0-10.3 us from a core of the
 * GPU's own NUMA node (profiles/r06/affinity_ahead_probe.txt) -- and an unpinned thread lands on either.
 * hc_device_local_cpus: the CPUs local to the device's PCIe root as the kernel lists them ("0-63,128-191"; "" when unknown).
 * hc_bind_thread_to_device: restricts the CALLING thread to those CPUs (sched_setaffinity; threads it creates afterwards inherit the
 * mask -- a host that wants its worker pool on all sockets creates it first, or binds only its stepping thread).  HC_ERR_UNSUPPORTED
 * when the CPUs are not known.  The worker threads of hc_step_multi bind themselves to their context's device (HC_MULTI_PIN=0: no). */
int hc_device_local_cpus(int device_id, char* out, size_t out_bytes);
int hc_bind_thread_to_device(int device_id);
int hc_create(int num_bodies, int device_id, hc_ctx** out);
/* Row-sharded context: owns output rows of bodies [body_begin, body_end) only. */
int hc_create_sharded(int num_bodies, int body_begin, int body_end, int device_id, hc_ctx** out);
void hc_destroy(hc_ctx* ctx);
/* The bodies [body_begin, body_end) whose output rows the context owns (either pointer may be NULL). */
int hc_get_shard(hc_ctx* ctx, int* body_begin, int* body_end);
const char* hc_last_error(const hc_ctx* ctx); /* ctx may be NULL: error of the last failed hc_create */

/* ------------------------------------------------------------------------------------------------
 * Ingest.  Replaces H5FileInfo::ReadH5Data (src/h5fileinfo.cpp:27-180); the raw-array setters take
 * exactly the datasets it reads, UNSCALED (the rho / rho*g scaling of :60-61,73-75,89-90 is applied
 * inside), so tests need no HDF5.
 * ---------------------------------------------------------------------------------------------- */
/* simulation_parameters/{rho,g,water_depth}  (src/h5fileinfo.cpp:35-37; "infinite" -> +inf, :207-220) */
int hc_set_simulation_parameters(hc_ctx* ctx, double rho, double g, double water_depth);
/* bodyK/properties/{disp_vol,cg,cb}  (:48,56-57) */
int hc_set_body_properties(hc_ctx* ctx, int body, double disp_vol, const double cg[3], const double cb[3]);
/* bodyK/hydro_coeffs/linear_restoring_stiffness {6,6}  (:58-59) */
int hc_set_hydrostatic_stiffness(hc_ctx* ctx, int body, const double lin[36]);
/* bodyK/hydro_coeffs/added_mass/inf_freq {6,D}  (:60-61) */
int hc_set_added_mass_inf(hc_ctx* ctx, int body, const double* A_6xD);
/* bodyK/hydro_coeffs/radiation_damping/impulse_response_fun/{t,K}; K is {6,D,S} (:49-50,62-63).
 * All bodies must carry the same t within 1e-10 (HydroData::GetRIRFTimeVector, :329-343). */
int hc_set_rirf(hc_ctx* ctx, int body, const double* t, int S, const double* K_6xDxS);
/* simulation_parameters/w and bodyK/hydro_coeffs/excitation/{mag,phase} {6,1,nw}  (:68-78) */
int hc_set_excitation_rao(hc_ctx* ctx, int body, const double* w, int nw, const double* mag_6x1xnw,
                          const double* phase_6x1xnw);
/* bodyK/hydro_coeffs/excitation/impulse_response_fun/{t,f}; f is {6,1,n}  (:83-90) */
int hc_set_excitation_irf(hc_ctx* ctx, int body, const double* t, int n, const double* f_6x1xn);
/* Reads all of the above for bodies "body1".."bodyN" from a BEMIO HDF5 file (needs libhdf5 at build
 * time, else HC_ERR_UNSUPPORTED). */
int hc_load_bemio_h5(hc_ctx* ctx, const char* path);
/* The same file WITHOUT a device context: H5FileInfo(path, num_bodies).ReadH5Data() (include/hydroc/h5fileinfo.h:230-260,
 * src/h5fileinfo.cpp:27-153) for callers that only want to look at the data (the reference's tests/h5fileinfo_t01.cpp,
 * chloadaddedmass_t01.cpp; the C++ face is include/hydroc_amd/h5fileinfo.h).  Host side only, no GPU is touched.  Values come back as the
 * reference's HydroData holds them: added mass x rho (:60-61), excitation magnitude x rho g (:73-75), excitation IRF x rho g (:89-90);
 * K, the stiffness matrix and everything else as in the file.  Errors: status code + hc_last_error(NULL). */
typedef struct hc_h5data hc_h5data;
int hc_h5_read(const char* path, int num_bodies, hc_h5data** out);
void hc_h5_free(hc_h5data* data);
/* S radiation samples, nw RAO frequencies, L excitation-IRF samples of (0-based) body `body`; any pointer may be NULL */
int hc_h5_get_sizes(const hc_h5data* data, int* num_bodies, double* rho, double* g, double* water_depth, int body, int* S, int* nw, int* L);
/* HydroData::BodyInfo (include/hydroc/h5fileinfo.h:37-47); ainf is {6, 6N} row-major, rirf_t has S entries; any pointer may be NULL */
int hc_h5_get_body(const hc_h5data* data, int body, double* disp_vol, double cg[3], double cb[3], double lin[36], double* ainf_6xD, double* rirf_t_S);
/* bodyK/.../impulse_response_fun/K in file order {6, 6N, S} (HydroData::GetRIRFVal(b, dof, col, s), src/h5fileinfo.cpp:321-323) */
int hc_h5_get_rirf(const hc_h5data* data, int body, double* K_6xDxS);
/* HydroData::RegularWaveInfo (:56-60): freq_list {nw}, magnitude {6, nw} x rho g, phase {6, nw} */
int hc_h5_get_excitation_rao(const hc_h5data* data, int body, double* w_nw, double* mag_6xnw, double* phase_6xnw);
/* HydroData::IrregularWaveInfo (:61-72): excitation_irf_time {L}, excitation_irf_matrix {6, L} x rho g */
int hc_h5_get_excitation_irf(const hc_h5data* data, int body, double* t_L, double* f_6xL);
/* End of ingest = rest of the TestHydro constructor (src/hydro_forces.cpp:176-238): trapezoid widths,
 * equilibrium, cb-cg, K re-laid-out into HBM, added-mass assembly (src/chloadaddedmass.cpp:12-25),
 * default NoWave. */
int hc_finalize(hc_ctx* ctx);

/* ------------------------------------------------------------------------------------------------
 * Configuration.
 * ---------------------------------------------------------------------------------------------- */
/* ChSystem::GetGravitationalAcceleration(), read by ComputeForceHydrostatics (src/hydro_forces.cpp:268).
 * Default (0,0,-9.81). */
int hc_set_gravity(hc_ctx* ctx, const double g[3]);
/* TestHydro::AddWaves(std::make_shared<NoWave>(num_bodies_arg))  (src/hydro_forces.cpp:244-261,
 * src/wave_types.cpp:257-264).  num_bodies_arg < N reproduces the reference's short force vector as an
 * error (HC_ERR_RUNTIME at the first step) instead of an out-of-bounds read. */
int hc_set_wave_none(hc_ctx* ctx, int num_bodies_arg);
/* AddWaves(RegularWave(num_bodies_arg)) with regular_wave_amplitude_/regular_wave_omega_
 * (src/wave_types.cpp:274-352). */
int hc_set_wave_regular(hc_ctx* ctx, int num_bodies_arg, double amplitude, double omega);

/* IrregularWaveParams (include/hydroc/wave_types.h:277-292); eta_file_path_ is hc_read_eta_file + hc_set_wave_irregular_eta below,
 * wave_stretching_ does not affect forces. */
typedef struct hc_irregular_wave_params {
    int num_bodies;
    double simulation_dt;
    double simulation_duration;
    double ramp_duration;
    double wave_height;
    double wave_period;
    double frequency_min;           /* default 0.001 */
    double frequency_max;           /* default 1.0   */
    double nfrequencies;            /* 0 = ceil((fmax-fmin)*duration) */
    double peak_enhancement_factor; /* 1.0 = Pierson-Moskowitz */
    int is_normalized;
    int seed;                       /* default 1 */
} hc_irregular_wave_params;
void hc_irregular_wave_params_default(hc_irregular_wave_params* p);
/* AddWaves(IrregularWaves(params)): excitation-IRF resampling, spectrum, phases, eta(t) table
 * (src/wave_types.cpp:432-459,572-606,643-676,717-774). */
int hc_set_wave_irregular(hc_ctx* ctx, const hc_irregular_wave_params* params);

/* AddWaves(IrregularWaves(params)) with params.eta_file_path_ set (src/wave_types.cpp:451-458): irregular waves from a measured or
 * precomputed free-surface elevation record instead of a spectrum.  The reference reads the record but convolves against a table
 * it never fills on that branch; the behaviour here is defined as follows (a deviation):
 *   record       t[0..n), n >= 2, finite and strictly increasing (spacing need not be uniform); eta[0..n) finite.  Used exactly as
 *                given: ramp_duration is not applied (as in ReadEtaFromFile).
 *   extension    eta(q) is the piecewise-linear interpolant of the record extended on both sides by eta = 0 samples spaced by the mean
 *                spacing h = (t[n-1] - t[0]) / (n-1): ceil(max(tau_max, 0) / h) + 1 before and ceil(max(-tau_min, 0) / h) + 1 after, for
 *                an excitation IRF on [tau_min, tau_max].  Forces are defined for every step time in [t[0], t[n-1]]; outside, the
 *                excitation-window error of hc_step applies.
 *   excitation   the IRF is resampled on the simulation_dt grid as by hc_set_wave_irregular; simulation_duration, the spectrum
 *                parameters and hc_set_eta_synthesis are ignored.
 *   queries      hc_get_eta_table returns the record as given (nt = n, without the zero extension); nf = 0, hc_get_spectrum returns
 *                nothing; hc_wave_kinematics returns zeros (the reference's kinematics over an empty spectrum), unless components
 *                are set (hc_set_eta_record_components below); hc_export_irregular_inputs_h5 gives HC_ERR_INVALID.
 * Row-sharded contexts take the whole record each. */
int hc_set_wave_irregular_eta(hc_ctx* ctx, const hc_irregular_wave_params* params, const double* t, const double* eta, int n);

/* Wave components of an imported eta record (not in the reference, whose record branch has no spectrum).  Opt-in: until this call
 * a record drives the excitation convolution and nothing else -- still water for hc_wave_kinematics, the Morison elements, the
 * nonlinear surface pressure, the QTF terms and the second-order sums -- with the bits it always had.  The call makes the record's
 * discrete Fourier coefficients on its own grid the component table (A, w, k, phi) that all of those read, so each of them runs
 * under a record through the kernels it has.  Valid only while the wave model is an imported record (else HC_ERR_INVALID).
 *   grid         n samples, h = (t[n-1] - t[0]) / (n-1), T_w = n h.  If |t[j] - (t[0] + j h)| <= 1e-9 h for every j the samples are
 *                used as given; otherwise the n values are those of the record's piecewise-linear interpolant (the one the
 *                excitation path reads) at t[0] + j h.  n >= 4.
 *   bins         f_m = m / T_w, 1 <= m <= floor(n / 2); the candidates are the bins with f_min_hz <= f_m <= f_max_hz (none:
 *                HC_ERR_INVALID).  The mean (m = 0) is never a component; the getter reports it.
 *   coefficient  c_m = (2 / n) sum_j eta_j exp(+i 2 pi ((m j) mod n) / n) on the GPU in FP64 (the Nyquist bin of an even n halved),
 *                the product m j reduced in 64-bit integers; one workgroup per bin with a fixed summation order, so a bin's bits
 *                depend on the record and on m only -- not on the band, on how many bins are computed, or on the shard.  The host
 *                turns c_m to the absolute time origin, c_m exp(i w_m t[0]), the product formed and reduced in long double;
 *                A_m = |c_m|, phi_m = arg c_m in the convention of hc_wave_kinematics: eta(0, t) = sum A cos(phi - w t).
 *   selection    max_components <= 0 keeps every candidate, else the max_components of largest A (ties: the lower m); the kept
 *                components are stored in ascending frequency.
 *   context      f = f_m, df = 1 / T_w, phase = phi_m, k from the dispersion relation at the context's depth and g as for a
 *                synthesised model; the component table takes A_m itself.  The call counts as a wave-model change for every cached
 *                component table and drops the wave directions, as every hc_set_wave_* call does; a later hc_set_wave_* call drops
 *                the components.  No ramp and no Wheeler stretching on the force terms (the record is used as given); the limits of
 *                the terms (component counts of the QTF and second-order sums) apply as to a synthesised sea.  hc_set_wave_directions
 *                accepts one uniform heading, as for hc_set_wave_irregular.  The excitation path is not touched: the record still
 *                drives the convolution, zero extension included, with the same bits.  Synchronous on the context's stream.
 *   LIMIT        the component sea is the PERIODIC continuation of the record with period T_w, while the excitation path has zeros
 *                outside [t[0], t[n-1]]: keep the side terms inside the record.  No window is applied.
 *   queries      hc_get_sizes reports nf = the kept count; hc_get_spectrum returns f, the one-sided periodogram A^2 / (2 df), df,
 *                phase and k; hc_export_irregular_inputs_h5 keeps refusing.
 * hc_clear_eta_record_components returns the record to its state before the call, bits included (HC_ERR_INVALID without a record;
 * nothing set: no effect).
 * hc_get_eta_record_components: *n = the kept count (0: none set); per kept component its bin m, f [Hz], A, phi and k; mean = the
 * mean of the analysed samples; variance_share = sum A^2 / 2 over their variance; rms_residual = the RMS of samples - mean -
 * reconstruction at the sample times (evaluated on the GPU with the exact integer phases).  Any pointer may be NULL (size query). */
int hc_set_eta_record_components(hc_ctx* ctx, double f_min_hz, double f_max_hz, int max_components);
int hc_clear_eta_record_components(hc_ctx* ctx);
int hc_get_eta_record_components(hc_ctx* ctx, int* n, int* m, double* f, double* amplitude, double* phase, double* k, double* mean,
                                 double* variance_share, double* rms_residual);
/* IrregularWaves::ReadEtaFromFile (src/wave_types.cpp:480-500) without a context: every line is `time : eta` (read as
 * `ss >> time >> delimiter >> eta`; the delimiter must be ':', what follows the value is ignored).  *n = number of samples;
 * t = eta = NULL: size query.  Errors (message in hc_last_error(NULL)): HC_ERR_RUNTIME "Unable to open file at: <path>." and
 * "Could not parse line: <line>." as the reference throws them; HC_ERR_OUT_OF_RANGE when capacity < *n (nothing copied). */
int hc_read_eta_file(const char* path, double* t, double* eta, int capacity, int* n);

/* How hc_set_wave_irregular builds the free-surface table eta(t) (GetEtaIrregularTimeSeries, src/wave_types.cpp:27-59):
 * 0 = direct FP64 sum of the Nf cosines per time sample on the GPU (default; same summation order as the reference),
 * 1 = chirp-z transform on rocFFT (three FFTs of length >= nt + nf - 1; agrees with the direct sum to ~1e-12 of max|eta|). */
int hc_set_eta_synthesis(hc_ctx* ctx, int mode);

/* Spectral (component-sum) excitation -- NOT in the reference (whose irregular waves are the excitation-IRF convolution
 * above); it is the mode BASELINE.json's north_star words literally: the same spectrum / phases as hc_set_wave_irregular,
 *   f[row](t) = ramp(t) * sum_i |X_row(w_i)| * a_i * cos(w_i t - phi_i + arg X_row(w_i)),   a_i = sqrt(2 S_i df_i),
 * with the excitation RAO interpolated per component by RegularWave's interpolator (src/wave_types.cpp:329-352, held
 * constant outside the BEM frequency range) and per-body phases.  Agrees with the IRF convolution up to the IRF's
 * truncation / resampling error (a few per cent on the sphere data), so it is validated at a looser tolerance.
 *   queries      hc_get_spectrum as for hc_set_wave_irregular; the mode has neither a resampled excitation IRF nor a free-surface
 *                table: hc_get_sizes gives L = 0 and nt = 0, hc_get_excitation_irf_size / _resampled give HC_ERR_INVALID,
 *                hc_get_eta_table succeeds and copies nothing (also on a context that held an IRF model's table before), and
 *                hc_export_irregular_inputs_h5 is refused with HC_ERR_INVALID (the file's free-surface datasets would be empty). */
int hc_set_wave_irregular_spectral(hc_ctx* ctx, const hc_irregular_wave_params* params);

/* TestHydro::SetRadiationConvolutionMode: 0 = Baseline, 1 = TaperedDirect (include/hydroc/hydro_forces.h:234-243) */
int hc_set_convolution_mode(hc_ctx* ctx, int mode);
/* TestHydro::TaperedDirectOptions (include/hydroc/hydro_forces.h:246-259) */
typedef struct hc_tapered_direct_options {
    int smoothing;                /* 0 = "sg" (Savitzky-Golay 5), 1 = "moving_average" */
    int window_length;            /* moving average only, >= 3 */
    double rirf_end_time;         /* <= 0: full length */
    double taper_start_percent;   /* 0.8 */
    double taper_end_percent;     /* 1.0 */
    double taper_final_amplitude; /* 0.0 */
    int export_plot_csv;          /* 0; 1: write rirf_body<b>_summary.csv (b 0-based, one per owned body; columns
                                     step,time,k_before,k_after of channel row 0 / column 0, src/hydro_forces.cpp:509-531) into the
                                     diagnostics directory when the kernel is processed */
} hc_tapered_direct_options;
void hc_tapered_direct_options_default(hc_tapered_direct_options* o);
int hc_set_tapered_direct_options(hc_ctx* ctx, const hc_tapered_direct_options* opts);
/* TestHydro::SetDiagnosticsOutputDirectory (include/hydroc/hydro_forces.h:269): where the export_plot_csv files go; "" (the
 * default) = the current working directory, as in the reference (src/hydro_forces.cpp:513).  Export errors are ignored (:529). */
int hc_set_diagnostics_output_directory(hc_ctx* ctx, const char* dir);

/* ------------------------------------------------------------------------------------------------
 * Per-step force evaluation.  Replaces the 6N ComponentFunc::GetVal -> ForceFunc6d::CoordinateFunc ->
 * TestHydro::CoordinateFuncForBody callbacks of one Chrono update (src/hydro_forces.cpp:79-85,136-144,
 * 727-767): total = hydrostatic - radiation + waves, evaluated once per distinct time `t` and cached.
 *   pos     [N][3]  ChBody::GetPos()
 *   rpy     [N][3]  ChBody::GetRot().GetCardanAnglesXYZ()
 *   linvel  [N][3]  ChBody::GetPosDt()
 *   angvel  [N][3]  ChBody::GetAngVelParent()
 *   force_out [D_local] world-frame force (x,y,z) and torque (x,y,z) per owned body.
 * Errors kept from the reference: excitation window exceeded (src/wave_types.cpp:833-840) -> HC_ERR_RUNTIME.
 * A step BACK in time (t below the newest history sample: an integrator that rejected a step and retries from an earlier time)
 * drops the history samples at times >= t -- they belong to the abandoned attempt -- and continues from the history as it was
 * at t.  Deviation: the reference has no such rule; it inserts the earlier time in front of its newest-first history
 * (src/hydro_forces.cpp:559-574), keeps the abandoned samples and interpolates in a non-monotone list from then on.
 * hc_step is synchronous (the forces are in force_out when it returns) but does not synchronise the stream: work that later
 * steps need may still be running on the context's stream.
 * ---------------------------------------------------------------------------------------------- */
int hc_step(hc_ctx* ctx, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel,
            double* force_out);
/* The two halves of hc_step for a host that has other work between handing the state to the GPU and needing the forces:
 * hc_step_begin stores the state, hands the step kernel to the GPU (and enqueues what later steps need) and returns;
 * hc_step_end waits for the results of that step.  Exactly one hc_step_end per hc_step_begin; no other per-step call on
 * the context in between.  Same cache and error rules as hc_step (a failure of either half leaves nothing pending). */
int hc_step_begin(hc_ctx* ctx, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel);
int hc_step_end(hc_ctx* ctx, double* force_out);
/* A prescribed-motion driver's loop ("the build's own counterpart is a mock Chrono loop"): n synchronous evaluations one
 * after the other -- hc_step(ctx, t_n[k], state k, force k) for k = 0 .. n-1 with state k the packed block
 * [pos 3N | rpy 3N | linvel 3N | angvel 3N] at states_nx12N + 12N*k and force k the D_local totals at forces_nxDlocal + D_local*k.
 * seconds_n (may be NULL) receives the wall time of every call (std::chrono::steady_clock around hc_step).  Stops at the first failing
 * step and returns its status; *done (may be NULL) is the number of steps completed.  Same results as n calls of hc_step: it is n calls. */
int hc_step_many(hc_ctx* ctx, int n, const double* t_n, const double* states_nx12N, double* forces_nxDlocal, double* seconds_n, int* done);
/* Multi-GPU inside ONE host process -- the reference is one C++ object in one Chrono process (src/hydro_forces.cpp:170-242),
 * evaluated by one call per time (:727-767); SURVEY 8e, drop-in variant.  ctxs[0..n_ctx) are row-sharded contexts of the same
 * N-body system (hc_create_sharded, any devices, any split of the bodies); the call stores the state into every context and
 * rings every GPU's doorbell BEFORE it enqueues anything else or waits, then gathers each shard's rows:
 *   force_out[6*body_begin(g) .. 6*body_end(g)) = the totals of context g          (force_out has 6N entries)
 * No collective, no device-to-device traffic: inputs are 12N doubles per GPU, outputs 6*n_local doubles per GPU, through the
 * PCIe BAR / mapped host memory like hc_step.  The gathered vector is bitwise the one an unsharded context returns.  On
 * failure the status of the first failing context is returned, hc_last_error() of every context of the group holds its
 * message, and no context is left with a step pending. */
int hc_step_multi(hc_ctx* const* ctxs, int n_ctx, double t, const double* pos, const double* rpy, const double* linvel,
                  const double* angvel, double* force_out);
/* One process per GPU (an MPI-style host, or this repo's benchmark under torch.distributed.run): the host gather without a collective.
 * hc_set_result_buffer makes the step kernel deliver this context's tagged results -- 16-byte {value, step sequence number} granules,
 * 2 x D_local of them, the two halves used by consecutive steps in turn -- into memory the caller provides, e.g. a POSIX
 * shared-memory segment every process of the node maps (the library registers it with the GPU; NULL returns to the internal buffer;
 * the memory must stay mapped until then or until hc_destroy).  `rows` of hc_wait_result_buffer = D_local of the shard that writes the buffer.
 * After hc_step_begin each process collects every shard's rows with hc_wait_result_buffer (host-only: it spins on the granules of the
 * given sequence number -- hc_step_sequence of the own context; contexts driven in lockstep count alike -- and copies the values
 * out; HC_ERR_DEVICE after timeout_seconds, <= 0: HC_STEP_TIMEOUT_S / 20 s), then completes its own step with hc_step_end. */
int hc_set_result_buffer(hc_ctx* ctx, void* host_buffer, size_t bytes);
int hc_step_sequence(const hc_ctx* ctx, unsigned long long* seq);
int hc_wait_result_buffer(const void* host_buffer, int rows, unsigned long long seq, double* values_out, double timeout_seconds);
/* Same evaluation with the body state already in HBM and the result left in HBM:
 *   d_state     device pointer, 12N doubles = pos[3N] | rpy[3N] | linvel[3N] | angvel[3N]
 *   d_force_out device pointer, D_local doubles
 *   stream      hipStream_t (NULL = the context's own stream).  Asynchronous: returns after enqueue; d_state and
 *               d_force_out must stay valid until the work enqueued for this step has run.  The steps of one context
 *               normally stay on one stream (the velocity ring is updated in stream order); a step that goes to another
 *               stream than the one before it -- hc_step included, which uses the context's stream -- is ordered behind
 *               it with an event.  hc_step and hc_step_device share the per-time cache.  On a caller's stream that is
 *               idle when the call arrives (a caller that waits for every step) only the step kernel is enqueued there;
 *               the work later steps need (scatter, look-ahead pass) runs on the context's own stream behind an event,
 *               and the next step waits for it -- what the caller enqueues next on its stream (e.g. the all-gather of the
 *               force rows of a row-sharded array) follows the step kernel directly.  A caller that enqueues steps ahead
 *               of the GPU gets all of it on its stream, in order. */
int hc_step_device(hc_ctx* ctx, double t, const double* d_state, double* d_force_out, void* stream);
/* force_hydrostatic_, force_radiation_damping_, force_waves_ of the last evaluated step (D_local each;
 * any pointer may be NULL).  Synchronises the context's stream. */
int hc_get_force_components(hc_ctx* ctx, double* hydrostatic, double* radiation, double* waves);
/* TestHydro::ComputeForceRadiationDampingConv called directly (src/hydro_forces.cpp:537-691): pushes
 * (t, velocities) into the history and returns the radiation term only.  Calling it twice with the
 * same t is the reference's duplicate-time error (:555-557) -> HC_ERR_RUNTIME. */
int hc_compute_radiation(hc_ctx* ctx, double t, const double* linvel, const double* angvel, double* rad_out);
/* TestHydro::ComputeForceHydrostatics (:263-322) and ComputeForceWaves (:713-725) on their own. */
int hc_compute_hydrostatics(hc_ctx* ctx, const double* pos, const double* rpy, double* hs_out);
int hc_compute_waves(hc_ctx* ctx, double t, double* waves_out);
/* Multi-step look-ahead (on by default, 32 steps): when the caller steps on a uniform time grid, one blocked pass over K
 * precomputes, for the next 32 (or 16) predicted step times, what the history known so far contributes to the radiation sum,
 * so K leaves HBM once per block; a step inside a block is ONE kernel launch that adds its own newest-sample part, and what
 * later steps of the block need from it is enqueued behind it (off the caller's critical path).  A step whose time deviates
 * from the prediction (> max(1e-9 of the step size, 64 ulp)) falls back to the plain per-step evaluation: a missed prediction
 * costs speed, never accuracy.  A step whose time is accepted is evaluated on the PREDICTED time grid (t0 + m*dt), so its
 * interpolation weights differ from those of the caller's t by at most that tolerance / dt relative (1e-15 .. 1e-12 observed;
 * contract 1e-6).  Wide systems (6N >= 1024) use a two-level form: sub-blocks of 8 steps with a short pass over the head of K
 * after each.  steps = 0 disables it (every step streams K), 1..16 selects blocks of 16, more blocks of 32 (a depth-64 pass exists in
 * the tuning build only: measured and not taken, EXPERIMENTS.md). */
int hc_set_lookahead(hc_ctx* ctx, int steps);
/* When the pass of a look-ahead block runs.  one_block_ahead < 0 (the default of every context): ADAPTIVE -- the library counts,
 * per block, how many of the gaps between the caller's synchronous steps (end of one hc_step / hc_step_multi to the begin of the
 * next) were longer than a threshold (HC_PASS_AHEAD_GAP_US; default 4 us, for wide systems 0 up to 12 GB of K in the context and a
 * tenth of the pass's cost per step above that) and runs the pass of the following block at block
 * start when the caller steps back to back, one block ahead when it is away between steps -- as a Chrono loop is; systems below
 * 256 MB of K (6N * 6N * S * 8 bytes) always run it at block start (their pass takes microseconds).  hc_step_multi measures the
 * gap once for its group of contexts, so the shards of one array decide alike.  The decisions are counted in
 * hc_profile_stats::schedule_blocks_ahead / schedule_blocks_at_start.
 * one_block_ahead = 0: when the block starts.  A caller that comes back before the pass has
 * finished waits for it on the first step of the block (190 us at 64 bodies; 1.55 ms for the 64-body row shard of a 512-body
 * array); a caller that stays away longer than that never notices it.  one_block_ahead = 1: the pass of the NEXT block is computed
 * from the history known when the current block starts, in `slices` launches (<= 0: chosen from the size of K, 2 .. 8) issued
 * behind the first steps of the current block, and what the current block's own samples add to the next block's steps follows in
 * short passes over the head of K.  With direct dispatch (and the device to itself) all of that runs BESIDE the steps, on a queue
 * of its own whose CU mask leaves a few compute units of every XCD to the step kernels; contexts that share a device, and steps
 * that go through HIP launches, issue the same launches on the step path's own queue / stream (the same sums; a back-to-back
 * caller then pays 10-30 % for them).  No step waits for a whole pass.
 * Measured on an MI355X, mean hc_step latency of a C++ caller with 30 / 100 / 300 us of host work between calls: 64 bodies
 * 18.9 -> 14.2 / 16.8 -> 14.1 / 14.0 -> 14.1 us (p99 at 30 us: 174 -> 19 us); the 64-of-512-body shard - / 66.8 -> 30.0 /
 * 60.1 -> 20.7 us (p99 at 300 us: 1306 -> 26 us).  A caller that steps back to back has nothing to hide the pass behind:
 * 19.5 -> 20.2 us at 64 bodies (the short pass towards the next block and the two queues sharing the chip), 74.7 -> 71.3 us for the shard.  Used once the history covers the IRF window; results are those of
 * schedule 0 up to the rounding of a different summation grouping (same 1e-6 contract, same tolerance on the predicted times).
 * The schedule is part of the configuration: the row shards of one array must use the same one (and the same slice count) to
 * stay bitwise equal to the unsharded context -- pin it (0 or 1) where that matters across separately driven contexts; under the
 * adaptive schedule two runs agree to rounding (1e-15), not bit for bit, when their callers' gaps differ.
 * HC_PASS_AHEAD=0/1 in the environment pins the default of new contexts (HC_PASS_CONCURRENT=0: no queue of its own); the slice count
 * is set through this call only.
 * REPRODUCIBILITY: with the schedule pinned (0 or 1) a run is bitwise repeatable whatever the caller's timing; under the adaptive
 * default it is repeatable to rounding ("Reproducibility"). */
int hc_set_pass_schedule(hc_ctx* ctx, int one_block_ahead, int slices);
/* Spectral radiation tail.  Where the step equals the IRF spacing, the history covers the IRF window on that grid, the look-ahead
 * depth is 16 or 32 and the pass of a block runs at block start, the older lags of the pass come from partitioned FFT convolutions
 * and the pass itself streams the first IRF samples of K only.  Systems with 6N >= 1024 and IRFs of fewer than 512 samples keep
 * the full pass.
 *   mode 1 (the default), in levels of doubling partition length: the lags 128 .. 255 once per 128 steps, 256 .. 511 once per 256
 *          steps and, for IRFs of 1024 samples and more, the lags from 512 on once per 512 steps (shorter IRFs: the lags from 256 on
 *          once per 256 steps); the pass streams the first 128 samples.  Fewest bytes per step; a step that starts a 512-step period
 *          waits for all levels' transforms of K to be streamed once.
 *   mode 2, uniform: the lags from 256 on once per 256 steps (a superblock), the pass streams the first 256 samples.
 *   mode 0: the full pass always.
 * The transform of K a mode needs (complex FP64, about 2 x S x 6N x 6N_loc x 8 bytes) is made at its first use and again after any
 * change of K, the taper or the convolution mode.  Results are those of mode 0 up to rounding.  Part of the configuration: the row
 * shards of one array must use the same mode. */
int hc_set_radiation_tail(hc_ctx* ctx, int mode);
/* What is in force: the look-ahead depth (0, 16 or 32: hc_set_lookahead clamps what it is given to what this build of the library
 * holds), the pass schedule (-1 adaptive, 0 at block start, 1 one block ahead), under the adaptive schedule the rule's current answer
 * (1: the next pass goes one block ahead), and the slice count of a pass made ahead.  Any pointer may be NULL.  For hosts that drive
 * the row shards of one array from several processes and want them to run ONE schedule: read it on one rank, pin it on all. */
int hc_get_schedule(const hc_ctx* ctx, int* lookahead, int* pass_schedule, int* ahead_now, int* slices);
/* How hc_step hands its kernels to the GPU.  1: as AQL packets written straight into an HSA queue of the library's own (kernel
 * arguments stored through the PCIe BAR) -- the default when the stand-alone code object hc_kernels.co lies next to the library,
 * the device's memory is host-addressable and the start-up self-tests pass (a dispatch completes; memory and argument slots the
 * host re-writes are re-read, not served stale); it saves the 2.4-3.3 us a hipLaunchKernelGGL call costs the host on the critical
 * path of every step (all kernels of hc_step / hc_step_begin / hc_step_multi and hc_added_mass_mv go this way, for systems of
 * every size).  0: through HIP launches on the context's stream (HC_DIRECT=0 forces this); hc_dispatch_mode_reason then says why.
 * Between steps of a caller that stays away for a while (a Chrono loop integrating) the library leaves its queue parked on a
 * barrier packet, so that the next step's kernel starts without the ~6 us an idle queue needs (HC_ARM=0 disables it).
 * A dispatch that never completes, or a queue the runtime reports broken, ends the wait after HC_STEP_TIMEOUT_S (default 20 s)
 * with HC_ERR_DEVICE; the context then fails every later step the same way.  The kernels and the results are the same either way.  hc_step_device always uses HIP,
 * and so does hc_step while hc_enable_profiling is on under a tool that intercepts HSA queues (rocprofv3): the tool sees direct
 * dispatches too, but the completion signals the library's own timings rest on are then the tool's. */
int hc_direct_dispatch_active(const hc_ctx* ctx);
const char* hc_dispatch_mode_reason(const hc_ctx* ctx);
/* Forget the velocity history and the per-time cache (fresh TestHydro state). */
int hc_reset_history(hc_ctx* ctx);
/* Injects a history as if those steps had been evaluated (times newest first, vel [n][D]); used to start
 * benchmarks in the steady state.  The only cross-step state of the path is this history plus the cached
 * time (checkpoint/resume). */
int hc_set_history(hc_ctx* ctx, int n, const double* times_newest_first, const double* vel_nxD);
int hc_get_history(hc_ctx* ctx, int* n, double* times_newest_first, double* vel_nxD); /* NULL arrays: size query */

/* ------------------------------------------------------------------------------------------------
 * Added mass.  Replaces ChLoadAddedMass (src/chloadaddedmass.cpp:12-70).
 * ---------------------------------------------------------------------------------------------- */
/* infinite_added_mass: D_local x D row-major, rho-scaled -- what ComputeJacobian puts top-left in M (:27-44) */
int hc_added_mass_matrix(hc_ctx* ctx, double* M_DlocalxD);
/* LoadIntLoadResidual_Mv: R[row0 + i] += c * sum_j M[i][j] * w[j], i < D_local (:55-70); w has >= D entries,
 * R has n_sys entries (n_sys >= D), row0 = 6*body_begin. */
int hc_added_mass_mv(hc_ctx* ctx, const double* w, double c, double* R_inout, int n_sys);
/* The same product for a row-sharded system held by n_ctx contexts of one process (see hc_step_multi): all shards are handed
 * to their GPUs first, then each shard's rows [6*body_begin, 6*body_end) of R are collected. */
int hc_added_mass_mv_multi(hc_ctx* const* ctxs, int n_ctx, const double* w, double c, double* R_inout, int n_sys);

/* ------------------------------------------------------------------------------------------------
 * Introspection (exporter / diagnostics parity).
 * ---------------------------------------------------------------------------------------------- */
/* HydroProfileStats (include/hydroc/hydro_forces.h:153-160), filled from HIP events; *_seconds are GPU
 * time of the kernels of each term.  conv_kernel_* describe the radiation GEMV kernel alone. */
typedef struct hc_profile_stats {
    /* HydroProfileStats: GPU seconds per term.  A launch that carries two terms (the convolution kernels stream K and,
     * for irregular waves, Kex) is apportioned by algorithmic bytes; hydrostatics_seconds is the step kernel (reduction,
     * the step's own newest-sample part, hydrostatics, regular / spectral wave term, total). */
    double hydrostatics_seconds, radiation_seconds, waves_seconds;
    int hydrostatics_calls, radiation_calls, waves_calls;
    double conv_kernel_seconds; /* sum of HIP-event durations of the plain per-step convolution launches */
    long long conv_kernel_launches;
    double conv_kernel_bytes;   /* algorithmic bytes of one step (8*D_local*D*S + vectors) */
    double block_kernel_seconds; /* look-ahead kernel launches (one covers a block of 32 or 16 steps) */
    long long block_kernel_launches;
    double block_kernel_bytes;  /* algorithmic bytes of the last pass: sum over its steps of the share of K (and of the
                                   velocity vector) that the pass computes for that step, i.e. IRF samples s >= s_cut[j] */
    double block_kernel_bytes_once; /* bytes the last LAUNCH of the pass kernel has to move once: live part of K, Kex, staged vectors
                                     * (the whole pass with the pass at block start, one slice of it under the schedule "one block
                                     * ahead"; block_kernel_bytes is scaled the same way) */
    double step_kernel_seconds;  /* the step kernel (finalize_kernel): the one launch on the critical path of a block step; wide
                                    systems (6N >= 1024): two launches per step, near_split_kernel + finalize_kernel, both counted */
    long long step_kernel_launches;
    double scatter_kernel_seconds; /* scatter launches (after a block step has delivered its forces) */
    long long scatter_kernel_launches;
    /* how the kernels of the per-step path reached the GPU since the last reset (counted whether or not profiling is on):
     * AQL packets written by the library itself / hipLaunchKernelGGL calls */
    long long direct_dispatches, hip_launches;
    long long history_rewinds;     /* steps back in time handled by dropping the newer history samples (see hc_step) */
    double mini_pass_seconds;      /* short passes of the two-level look-ahead of wide systems (one per sub-block of 8 steps) */
    long long mini_pass_launches;
    long long queue_parkings;      /* times the direct queue was left parked on a barrier packet after a step / an added-mass product */
    long long ahead_pass_slices;   /* pass schedule "one block ahead": launches of passes of a NEXT block (counted in block_passes too) */
    long long ahead_blocks;        /* ... and blocks that started with their rows already there (no pass at block start) */
    long long pass_lane_launches;  /* passes / short passes dispatched to the pass lane of the direct queue (they run beside the steps) */
    /* hc_step_multi: when this context's step kernel was handed to its GPU, measured from the entry of the call (seconds; the value
     * of the last call, the sum over all calls and their number) -- the fan-out cost of a multi-GPU step as each GPU sees it */
    double multi_doorbell_offset_last, multi_doorbell_offset_sum;
    long long multi_calls;
    long long slot_state_steps;    /* steps whose body state travelled behind the step kernel's argument block (direct dispatch, one-launch steps
                                    * of systems of up to 170 bodies, i.e. every system that is not wide): the kernel requests it together with its arguments, not after them */
    long long wide_fused_steps;    /* block steps of a wide system (6N >= 1024) whose own-sample slices and step kernel went out as ONE launch (wide_step_kernel) */
    long long schedule_blocks_ahead, schedule_blocks_at_start; /* look-ahead blocks at whose start the pass schedule answered "the pass of
                                    * the NEXT block runs one block ahead" / "at block start" (hc_set_pass_schedule; under the adaptive
                                    * schedule this is the rule's answer block by block) */
    long long ring_grows_for_pass; /* times the history ring was re-allocated so that a pass one block ahead can read its view of the
                                    * history while the block's steps push their samples (steps well below the IRF spacing) */
    long long hot_steps;           /* of slot_state_steps: block steps that went to the step kernel of the common case (step_hot_kernel: the
                                    * step's own IRF samples against its own velocity only, no plain partials, no spectral wave mode) */
    /* spectral radiation tail (hc_set_radiation_tail): launches of its kernels (forward transforms, frequency-domain products,
     * inverse transforms of every level), their GPU time where it was measured, the bytes they move, and the look-ahead blocks whose
     * older lags came from it.  block_kernel_* above then count the head pass (lags below 128, mode 2: below 256) alone. */
    long long tail_launches;
    double tail_seconds;
    double tail_bytes;
    long long tail_blocks;
} hc_profile_stats;
/* HIP events around the kernels of every `on`-th step (on = 1: every step; 0: off, the default), and around every
 * look-ahead pass (one per block) whatever the stride.  Event records perturb the launch stream by a few
 * microseconds, so throughput runs should sample (e.g. on = 17). */
int hc_enable_profiling(hc_ctx* ctx, int on);
int hc_get_profile(hc_ctx* ctx, hc_profile_stats* out);
int hc_reset_profile(hc_ctx* ctx);

/* What the INIT half of the path cost this context (seconds of host wall clock unless stated; GPU kernels by HIP events), stage by
 * stage, with the bytes each stage has to move -- so that a host (and bench.py's `init` block) can put every stage beside its
 * bound: the HDF5 reads beside the file size, the staging copies beside the PCIe rate, the re-layout / TaperedDirect / generator
 * kernels beside the HBM rate, the free-surface synthesis beside the FP64 rate.  Accumulated since hc_create. */
typedef struct hc_init_stats {
    double h5_read_seconds, h5_read_bytes;             /* hc_load_bemio_h5: HDF5 reads (datasets this context reads) */
    double rirf_h2d_seconds, rirf_h2d_bytes;           /* radiation IRF tensors {6, 6N, S} per owned body, pageable host memory -> HBM staging */
    double rirf_relayout_seconds, rirf_relayout_bytes; /* relayout_rirf_kernel: file order -> panel layout, rho folded in (bytes read + written) */
    double finalize_seconds;                           /* hc_finalize: widths, hydrostatic tables, added mass, buffers, direct-dispatch set-up + self-tests */
    double direct_setup_seconds;                       /* ... of which the direct-dispatch set-up (code object, queues, self-tests) */
    double wave_resample_seconds;                      /* hc_set_wave_irregular: excitation-IRF resample (LinSpaced + cubic B-spline, host) */
    double wave_spectrum_seconds;                      /* ... spectrum, phases, wavenumbers (host) */
    double wave_eta_seconds;                           /* ... free-surface table on the GPU: eta_kernel (direct FP64 sum) or the rocFFT chirp-z form */
    long long wave_eta_samples, wave_eta_components;   /* nt, nf of that table */
    int wave_eta_mode, pad_;                           /* 0 direct sum, 1 rocFFT */
    double wave_upload_seconds, wave_upload_bytes;     /* ... Kex re-layout, table uploads, read-back of eta */
    double wave_total_seconds;                         /* ... the whole call */
    double taper_seconds, taper_bytes;                 /* TaperedDirect preprocessing (taper_kernel; bytes read + written) */
    double synth_seconds, synth_bytes;                 /* hc_synth_fill: the generator kernel (bytes written) */
} hc_init_stats;
int hc_get_init_stats(const hc_ctx* ctx, hc_init_stats* out);

/* Sizes: S radiation samples, L resampled excitation samples, nf wave components, nt eta samples,
 * H current history length, Hcap ring capacity. Any pointer may be NULL. */
int hc_get_sizes(hc_ctx* ctx, int* N, int* n_local, int* S, int* L, int* nf, int* nt, int* H, int* Hcap);
/* rirf_width_vector (src/hydro_forces.cpp:181-190) */
int hc_get_rirf_width(hc_ctx* ctx, double* w_S);
/* The kernel actually convolved, mapped back to reference indexing: value = GetRIRFval(row, col, s)
 * (src/hydro_forces.cpp:693-711), i.e. rho-scaled and, in TaperedDirect mode, processed (:385-535).
 * rows are local; out is [D_local][D][S].  Meant for small cases. */
int hc_get_rirf_effective(hc_ctx* ctx, double* out_DlocalxDxS);
/* One value of the same: TestHydro::GetRIRFval(row, col, st) (src/hydro_forces.cpp:693-711) for a LOCAL row; indices outside
 * [0, D_local) x [0, D) x [0, S) give HC_ERR_OUT_OF_RANGE (the reference throws std::out_of_range, :694-697). */
int hc_get_rirf_value(hc_ctx* ctx, int row_local, int col, int st, double* out);
/* ex_irf_time_sampled_, ex_irf_width_sampled_, ex_irf_sampled_ (6 x L) of a local body (src/wave_types.cpp:572-628) */
int hc_get_excitation_irf_resampled(hc_ctx* ctx, int body, double* t_L, double* width_L, double* vals_6xL);
/* Bodies may carry different excitation-IRF time grids (the reference keeps one per body, src/wave_types.cpp:432-459): L of this
 * body's resampled grid (hc_get_sizes reports the sum over the distinct grids = the columns of the excitation matrix). */
int hc_get_excitation_irf_size(hc_ctx* ctx, int body, int* L);
/* spectrum_frequencies_, spectral_densities_, spectral_widths_, wave_phases_, wavenumbers_ (:643-676) */
int hc_get_spectrum(hc_ctx* ctx, double* f, double* S, double* df, double* phase, double* k);
/* free_surface_time_sampled_ / free_surface_elevation_sampled_ (:717-774; exporter: runner:668-679) */
int hc_get_eta_table(hc_ctx* ctx, double* t_nt, double* eta_nt);
/* SimulationExporter::WriteIrregularInputs (src/simulation_exporter.cpp:365-393): writes frequencies_hz, spectral_densities,
 * free_surface_time, free_surface_eta (+ the reference's attributes) under /inputs/simulation/waves/irregular of an HDF5
 * result file (created if absent).  Needs libhdf5 (HC_ERR_UNSUPPORTED otherwise). */
int hc_export_irregular_inputs_h5(hc_ctx* ctx, const char* path);
/* RegularWave::excitation_force_mag_/phase_ and wavenumber_ (:278-299) */
int hc_get_regular_coeffs(hc_ctx* ctx, double* mag_D, double* phase_D, double* wavenumber);
/* rho, g, water_depth of the context (hc_set_simulation_parameters / the HDF5 file): what WaveBase::AddH5Data copies into
 * g_ and water_depth_ (src/wave_types.cpp:280-281,509-510).  Any pointer may be NULL. */
int hc_get_simulation_parameters(hc_ctx* ctx, double* rho, double* g, double* water_depth);

/* ------------------------------------------------------------------------------------------------
 * Wave kinematics: WaveBase::GetElevation / GetVelocity / GetAcceleration (include/hydroc/wave_types.h:69-73) of the wave model
 * in force, batched over points x times, on the GPU.  Per component (A, w, k, phi) at x = position.x, z' = position.z - mwl:
 * eta = A cos(k x - w t + phi) (src/wave_types.cpp:14-44); velocity / acceleration (:61-158) with the exponential profile when
 * 2 pi / k > depth || k depth > 500, else cosh / sinh (k (z' + depth)) / sinh(k depth); y components 0.
 *   RegularWave (:301-313): one component, phi = regular_phase, no stretching.
 *   IrregularWaves (:515-550, both hc_set_wave_irregular and hc_set_wave_irregular_spectral): the sum over the spectrum in
 *   index order, A_i = sqrt(2 S_i df_i), w_i = 2 pi f_i; with wave_stretching the kinematics are evaluated at
 *   z_s = depth (z' - eta) / (depth + eta) (Wheeler), from which the profile subtracts mwl once more, as the reference does; for
 *   an infinite depth (where the reference gives NaN) at the limit z_s = z' - eta.
 *   NoWave (include/hydroc/wave_types.h:103-109), or no wave model: zeros, no launch.
 *   An imported eta record: zeros, no launch, unless components are set (hc_set_eta_record_components): then the sum over them,
 *   with stretching as the options say.
 * Not ramped (the eta(t) table is; kinematics are not).  Without directions (hc_set_wave_directions below) the sea runs along +x
 * and only x enters the phase, as in the reference, which ignores waves.direction; with directions every component has its own
 * and y enters as well.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hc_wave_kinematics_opts {
    double mwl;            /* WaveBase::mwl_ (0) */
    double regular_phase;  /* RegularWave::regular_wave_phase_ (0) */
    int wave_stretching;   /* IrregularWaveParams::wave_stretching_ (1) */
} hc_wave_kinematics_opts;
void hc_wave_kinematics_opts_default(hc_wave_kinematics_opts* o);
/* xyz[n_points][3], t[n_times] -> eta[T][P], vel[T][P][3], acc[T][P][3]; any output may be NULL, o NULL = the defaults.
 * Synchronous on the context's stream; needs hc_finalize.  Counts must be >= 0 and a pointer is required where its count is > 0;
 * non-finite x, z or t (and y while wave directions are set), non-finite options, or more than 2^31 - 256 (point, time) pairs give HC_ERR_INVALID.  Every output sums
 * the components in index order on its own, so its bits do not depend on the batch it is part of, nor on which shard context of
 * the system answers.  Changes no force and no step state. */
int hc_wave_kinematics(hc_ctx* ctx, const hc_wave_kinematics_opts* o, int n_points, const double* xyz,
                       int n_times, const double* t, double* eta, double* vel, double* acc);

/* ------------------------------------------------------------------------------------------------
 * Wave heading and short-crested seas (not in the reference, which parses waves.direction and ignores it: src/wave_types.cpp:20,34):
 * one direction per component of the wave model in force, the single-direction-per-frequency ("equal-energy") method.  Opt-in; with
 * no directions set every result keeps the bits it had.  theta_i in radians, 0 along +x, positive towards +y.  Per component, with
 * psi_i = k_i (x cos theta_i + y sin theta_i) - w_i t + phi_i:
 *     eta = sum A_i cos psi_i,   u_h = w A p_x cos psi_i,   velocity = (u_h cos theta_i, u_h sin theta_i, w A p_z sin psi_i),
 *     a_h = w^2 A p_x sin psi_i, acceleration = (a_h cos theta_i, a_h sin theta_i, -w^2 A p_z cos psi_i)
 * with the profiles p_x, p_z, the stretching, the mwl rule, the infinite-depth limit and the ramps of the long-crested sums.
 * hc_wave_kinematics, the Morison elements and the nonlinear surface forces (panels and clipped triangles) sample this sea.
 *
 * hc_set_wave_directions: n = the component count (1 for a regular wave, nf for hc_set_wave_irregular and
 * hc_set_wave_irregular_spectral); n == 0 or theta == NULL clears the directions.  HC_ERR_INVALID: a wrong n, a non-finite angle,
 * NoWave, no model or an imported eta record (no components, unless components are set), a direction outside a body's heading grid, or non-uniform directions
 * on the spectral model while a local body has no heading tables.  HC_ERR_UNSUPPORTED: non-uniform directions on the IRF model of
 * hc_set_wave_irregular -- its excitation is one convolution of eta(0, t), which a spread sea does not have: use
 * hc_set_wave_irregular_spectral.  A uniform heading is accepted there; the caller's excitation IRF is then understood to be the one
 * of that heading, and no step state is touched.  A failed call changes nothing.
 * EVERY hc_set_wave_* call that succeeds drops the directions (the component count changes with the model): set the wave model
 * first, then the directions.  A call that fails on its arguments leaves the model in force, its directions and the excitation
 * tables built for them as they were.
 * hc_get_wave_directions: *n = the count (0: none set); theta may be NULL (size query).
 *
 * What refuses while directions are set (HC_ERR_UNSUPPORTED from the compute / begin call, nothing stays pending; as before once
 * they are cleared): hc_wave_kinematics2 (hc_wave_kinematics2_dir is the call for this sea); the Morison elements on the
 * second-order sea (hc_set_morison_second_order with `on`) unless hc_set_morison_second_order_directional is on, which makes them
 * see the increments of hc_wave_kinematics2_dir; the nonlinear surface on the second-order sea (hc_set_nonlinear_second_order with
 * `on`) unless hc_set_nonlinear_second_order_directional is on, which gives it eta2 and q2 of that sea; and hc_drift_begin with a drift mode != 0 / hc_sum_qtf_begin with a sum mode != 0 while
 * some body of the system holds a one-heading table of that term (hc_set_drift_qtf, hc_set_sum_qtf): their pair sums and those
 * tables are of one long-crested heading.  QTF tables on a heading grid (hc_set_drift_qtf_headings, hc_set_sum_qtf_headings) are
 * evaluated.
 *
 * First-order excitation under a heading: hc_set_excitation_rao_headings gives a body its excitation coefficients on a grid of
 * headings, dir_rad[n_dir] strictly increasing, mag / phase [6][n_dir][nw] (the layout of a BEMIO file; magnitudes per rho g as for
 * hc_set_excitation_rao); n_dir == 0 removes them; allowed before and after hc_finalize.  While directions are set on the spectral
 * model or on a regular wave, the per-row x per-component (magnitude, phase) table of every body with heading tables is the omega
 * interpolation of that model at the two bracketing headings, then linear in the heading on the phases as given; a direction on a
 * grid node has weight exactly 0 on its neighbour.  No extrapolation and no wrap-around: a caller who wants the full circle supplies
 * both ends.  A body without heading tables keeps its {6,1,nw} table under a uniform heading.  The tables are replaced under the
 * synchronisation of hc_set_wave_irregular_spectral (the look-ahead excitation rows are dropped).
 *
 * hc_wave_spreading_directions needs no context: equal-energy directions of the cos-2s spreading
 * D(theta) ~ cos^{2s}((theta - heading) / 2) on (heading - pi, heading + pi).  Bin m of n_bins has direction
 * heading + G^-1((m + 1/2) / n_bins), G the cumulative distribution of D; every run of n_bins consecutive components takes every
 * bin once, in a permutation drawn from `seed` by a counter-based generator (the same output on every platform).  s <= 0 or
 * n_bins == 1: theta_i = heading.  HC_ERR_INVALID: nf < 0, n_bins < 1, non-finite heading or s, NULL output with nf > 0.
 * ---------------------------------------------------------------------------------------------- */
int hc_set_wave_directions(hc_ctx* ctx, int n, const double* theta_rad);
int hc_get_wave_directions(hc_ctx* ctx, int* n, double* theta_rad);
int hc_set_excitation_rao_headings(hc_ctx* ctx, int body, int n_dir, const double* dir_rad, const double* w, int nw,
                                   const double* mag_6xndirxnw, const double* phase_6xndirxnw);
int hc_get_excitation_rao_headings_size(hc_ctx* ctx, int body, int* n_dir, int* nw);
int hc_wave_spreading_directions(int nf, double heading_rad, double s, int n_bins, unsigned long long seed, double* theta_out);

/* ------------------------------------------------------------------------------------------------
 * Morison drag and inertia elements (not in the reference, which has none: src/hydro_types.h:34): an opt-in additional force
 * term on the wave kinematics above.  Element e of a body: position r in the body frame (relative to the point pos[b] locates),
 * cd_area_i = Cd_i A_i [m^2] and cm_vol_i = Cm_i V [m^3] per BODY axis (1 + Ca for a member outside the BEM mesh, 0 for drag only).
 * With the state of hc_step:
 *     R = Rx(rpy0) Ry(rpy1) Rz(rpy2) (Cardan XYZ),  d = R r,  p = pos + d,  v_e = linvel + angvel x d
 *     eta, u_f, a_f = hc_wave_kinematics at p and t with the Morison options; for the two synthesised irregular models u_f and a_f
 *         are multiplied by the ramp of hc_set_wave_irregular_spectral (ramp_duration > 0 and t < ramp_duration: 0 for t <= 0, else
 *         t / ramp_duration; its derivative is not added); a regular wave is not ramped; NoWave, no model or an imported eta
 *         record: still water (eta = u_f = a_f = 0), unless components are set (hc_set_eta_record_components): then the sea of
 *         those components, not ramped and not stretched
 *     wet when p.z - mwl <= eta; a dry element contributes nothing
 *     u = R^T (u_f - v_e),  a = R^T a_f,  F_body,i = 1/2 rho cd_area_i |u_i| u_i + rho cm_vol_i a_i,  F = R F_body,  M = d x F
 * A body's 6-vector is the sum of (F, M) over its elements in element index order: world frame, at the body reference, the sign of
 * an applied force.  Its bits depend on that body's state and elements, the wave model, t and the options only -- not on the number
 * of bodies, on other bodies' elements, or on the shard context that computes it.  The body-acceleration term of Morison's equation
 * is not included (the step inputs carry no acceleration).
 *
 * The term is NOT part of hc_step & co., hc_get_force_components or hc_compute_*: a caller adds it to the total (the HydroForces /
 * TestHydro layers do).  It runs on a stream of its own, beside the steps, and touches no step state: hc_morison_begin may be
 * followed by hc_step and then hc_morison_end.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hc_morison_element {
    double r[3];
    double cd_area[3];
    double cm_vol[3];
} hc_morison_element;
/* Replaces the list of `body` (0-based, any body of the system; a shard context computes those of its own bodies); n = 0 clears
 * it.  Before or after hc_finalize, between steps.  HC_ERR_INVALID: body out of range, n < 0, a null list with n > 0, a non-finite
 * value, a negative coefficient, more than 4096 elements, or a hc_morison_begin without its end. */
int hc_set_morison_elements(hc_ctx* ctx, int body, const hc_morison_element* elems, int n);
int hc_get_morison_count(hc_ctx* ctx, int body, int* n);
/* mwl, regular_phase, wave_stretching of the kinematics the elements see; NULL = the defaults */
int hc_set_morison_options(hc_ctx* ctx, const hc_wave_kinematics_opts* o);
/* begin enqueues (state as for hc_step: [3N] each), end waits and copies the 6 * n_local values of the owned bodies; exactly one
 * end per begin.  Needs hc_finalize.  HC_ERR_INVALID on a non-finite state or t, on a second begin, on an end without a begin;
 * nothing stays pending after a failure.  With no element and no strip member (hc_set_morison_members, below) on any owned body:
 * zeros, no launch. */
int hc_morison_begin(hc_ctx* ctx, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel);
int hc_morison_end(hc_ctx* ctx, double* out_Dlocal);
int hc_compute_morison(hc_ctx* ctx, double t, const double* pos, const double* rpy, const double* linvel, const double* angvel,
                       double* out_Dlocal);

/* Morison elements on the second-order sea: with `on` the elements see the second-order increments of Sharma and
 * Dean's long-crested sea (hc_wave_kinematics2, below) on top of the first-order field.  For element e, with R, d, p, v_e as above:
 *     eta1, u1, a1 = the values above: hc_wave_kinematics at p, t with the Morison options, stretching by eta1 included, u1 and a1
 *         times the Morison ramp
 *     eta2, u2, a2 = hc_wave_kinematics2 at the same FP64 point p and time t, with mwl and regular_phase of the Morison options
 *         (hc_set_morison_options) and the four cut-offs [rad/s] and apply_ramp of this call; everything else of that definition
 *         applies as written there: fields held at z2 = min(z - mwl, 0) and at -h below the bed, no stretching, the true depth,
 *         ramp * ramp on all three increments (eta2 included) with apply_ramp
 *     eta = eta1 + eta2,  u_f = u1 + u2,  a_f = a1 + a2;  wet when p.z - mwl <= eta;  the force formula is unchanged
 * NoWave, no wave model, an imported eta record (unless components are set), or cut-offs that leave no pair inside either band: no second-order launch, the
 * result is that of order 1 bit for bit.  With on = 0 (the default) every Morison call makes the launches and returns the bits it
 * did before this switch existed.  The increments of an element are those hc_wave_kinematics2 returns for its point, bit for bit;
 * a body's bits still depend on that body's state and elements, the wave model, t and the options only.
 * The pair tables and band limits are this path's own, built on its stream and cached on the wave model, the regular phase and the
 * cut-offs: a second copy beside the one hc_wave_kinematics2 keeps (4 nf^2 doubles: 8 MB at 512 components, 537 MB at 4096), freed
 * by on = 0.  HC_ERR_INVALID: a negative or NaN cut-off, lo > hi, or a hc_morison_begin without its end.  More than 4096 wave
 * components: hc_morison_begin returns HC_ERR_UNSUPPORTED and nothing stays pending.
 * Not included (out of scope): stretching of the second-order part.  The surface panels and triangles have a switch of their own
 * (hc_set_nonlinear_second_order, and hc_set_nonlinear_second_order_directional in a short-crested sea); the drift term stays first
 * order. */
int hc_set_morison_second_order(hc_ctx* ctx, int on, double diff_lo, double diff_hi, double sum_lo, double sum_hi, int apply_ramp);
int hc_get_morison_second_order(hc_ctx* ctx, int* on, double* diff_lo, double* diff_hi, double* sum_lo, double* sum_hi, int* apply_ramp);
/* The same in a short-crested sea.  While hc_set_morison_second_order is on and wave directions are set
 * (hc_set_wave_directions; a uniform heading on the IRF model included), hc_morison_begin answers HC_ERR_UNSUPPORTED unless this
 * switch is on (default 0).  With it on, element e sees eta = eta1 + eta2 in the wet test and u_f = ramp u1 + u2,
 * a_f = ramp a1 + a2 with all three components, where eta1, u1, a1 are the directional first-order values (hc_set_wave_directions:
 * Morison options, stretching by eta1) and eta2, u2, a2 are what hc_wave_kinematics2_dir returns for the same FP64 point p and time,
 * bit for bit, with mwl and regular_phase of the Morison options and the four cut-offs and apply_ramp of
 * hc_set_morison_second_order.  The force formula is the directional first-order one.  The pair tables are those of the directional
 * pair sum, again this path's own (not shared with hc_wave_kinematics2_dir's; the one set of this path holds either kind, rebuilt
 * when the directions come or go); on = 0 of hc_set_morison_second_order frees them.  The rules above carry over: no components or
 * no pair inside either band -- no second-order launch and the directional first-order bits; more than 4096 components --
 * HC_ERR_UNSUPPORTED from hc_morison_begin; a body's bits depend on that body's state and elements, the wave model with its
 * directions, t and the options only.
 * The switch is independent of hc_set_morison_second_order: it keeps its value when that one goes off and on, has no effect while
 * that one is off, and none without directions (the long-crested path, its kernels and its bits).  HC_ERR_INVALID: a
 * hc_morison_begin without its end. */
int hc_set_morison_second_order_directional(hc_ctx* ctx, int on);
int hc_get_morison_second_order_directional(hc_ctx* ctx, int* on);
/* What the elements of `body` (0-based, owned by this context) saw in the last completed evaluation that had a second-order part:
 * their points p[n][3] and the increments eta2[n], vel2[n][3], acc2[n][3], n = the body's element count at that evaluation.  After a
 * directional evaluation vel2[.][1] and acc2[.][1] carry u2y and a2y; after a long-crested one they are 0.  Any pointer may be NULL.  HC_ERR_INVALID: second order is off, no such evaluation has completed yet (one without a
 * second-order part -- no components, empty bands, no element on an owned body -- forgets the one before, and so does
 * hc_set_morison_elements), or the body is not owned by this context. */
int hc_get_morison_increments(hc_ctx* ctx, int body, double* p, double* eta2, double* vel2, double* acc2);

/* Morison strip members (DESIGN.md 3.7c'): a slender cylinder given as OpenFAST and WEC-Sim give it -- two end points, a diameter
 * at each, Cd and Cm -- integrated along its wet length.  The drag acts along the flow component normal to the member's axis, so an
 * inclined member is right for every flow direction, and the member is cut at the instantaneous free surface, so the force is
 * continuous in the draft.  With R, d = R r, p = pos + d, v_e = linvel + angvel x d exactly as the elements define them, the state
 * of hc_step and the options of hc_set_morison_options:
 *     nodes      j = 0..n_seg at r_j = r0 + (j / n_seg)(r1 - r0), P_j = pos + R r_j;  eta_j = the first-order elevation
 *                hc_wave_kinematics returns at (P_j, t) with the Morison options (the directional sea while hc_set_wave_directions
 *                holds, still water where the elements have still water);  h_j = P_j.z - mwl - eta_j;  the node is wet iff h_j <= 0
 *     segment    (nodes j, j + 1, local sigma in [0, 1] from node j), h taken as linear along it: both nodes wet -- the wet part is
 *                [0, 1]; both dry -- nothing; else one cut at sigma* = h_x / (h_x - h_y) measured from the wet end x (h_x <= 0 < h_y):
 *                the wet part [sigma_a, sigma_b] is [0, sigma*] when node j is the wet one and [1 - sigma*, 1] when node j + 1 is
 *     quadrature two Gauss-Legendre points per wet segment, sigma_g = sigma_a + (sigma_b - sigma_a)(1/2 -+ 1/(2 sqrt 3)), weight
 *                w_g = 1/2 (sigma_b - sigma_a) |r1 - r0| / n_seg (exact for a cubic load per length, so for a constant one at any n_seg)
 *     per point  s = (j + sigma_g) / n_seg, r_g = r0 + s (r1 - r0), D_g = d0 + s (d1 - d0);  d, p, v_e as above;  u_f, a_f = what an
 *                element at p sees: hc_wave_kinematics at (p, t) with the Morison options, Wheeler stretching by the point's own
 *                eta when it is on, times the Morison ramp; no second wet test at the point;  with the unit axis
 *                a^ = R (r1 - r0) / |r1 - r0|:  q = u_f - v_e,  q_n = q - (q . a^) a^,  a_n = a_f - (a_f . a^) a^,
 *                dF = w_g [1/2 rho cd D_g |q_n| q_n + rho cm (pi / 4) D_g^2 a_n],  dM = d x dF
 * A member's 6-vector is the serial sum of its Gauss points (segment order, the lower point first); a body's member vector is the
 * serial sum of its members in index order: hc_get_morison_member_forces returns the first level [n][6], and summing its rows
 * serially in FP64 reproduces the second bit for bit.  hc_morison_end / hc_compute_morison return, per component, elements + members
 * with one IEEE addition for a body that carries members, and exactly the bits they returned before for a body that carries none.
 * A body's bits depend on that body's state, its own member list, the wave model with its directions, t and the options only.
 * Members see the first-order sea unless hc_set_morison_members_second_order (below) is on: while hc_set_morison_second_order is
 * on, that switch is off and an owned body carries members, hc_morison_begin answers HC_ERR_UNSUPPORTED and nothing stays pending.
 * Not included: axial (end-cap) drag and added mass, which stay point elements; MacCamy-Fuchs diffraction.  The body-acceleration
 * term comes as a matrix: hc_set_morison_member_added_mass (below). */
typedef struct hc_morison_member {
    double r0[3], r1[3]; /* end points in the body frame, relative to the point pos[b] locates [m]; r0 != r1 */
    double d0, d1;       /* diameter at r0 and at r1 [m], linear in between; >= 0 */
    double cd;           /* transverse drag coefficient, >= 0 */
    double cm;           /* transverse inertia coefficient (1 + Ca outside the BEM mesh, Ca or 0 inside), >= 0 */
    int n_seg;           /* segments along the member, 1..64 */
} hc_morison_member;     /* 88 bytes */
/* Replaces the member list of `body` (0-based, any body of the system); n = 0 clears it; at most 1024 per body.  HC_ERR_INVALID: body
 * out of range, n < 0, a null list with n > 0, a non-finite value, a negative diameter or coefficient, r0 == r1, n_seg outside
 * 1..64, more than 1024 members, or a hc_morison_begin without its end. */
int hc_set_morison_members(hc_ctx* ctx, int body, const hc_morison_member* members, int n);
int hc_get_morison_member_count(hc_ctx* ctx, int body, int* n);
/* The 6-vectors of the members of `body` in the last completed evaluation, [n][6].  HC_ERR_INVALID: a body this context does not
 * own, a null output, or no evaluation with members completed since a member list was last set. */
int hc_get_morison_member_forces(hc_ctx* ctx, int body, double* out_nx6);

/* Strip members: the added-mass matrix on the instantaneous wet length (DESIGN.md 3.7c''').  The body-acceleration term of
 * Morison's equation, -rho Ca V a_body, needs an input the step does not carry, so it is handed over in the form an integrator
 * wants: a 6 x 6 matrix per body, as the BEM added mass is (hc_added_mass_matrix).  Each member has a coefficient ca >= 0, default
 * 0, set beside the list.  R, d = R r_g, the nodes, h_j, the wet interval, the Gauss points, w_g, D_g and a^ are exactly those of the
 * member force in the same evaluation -- eta2 in h_j included while hc_set_morison_members_second_order applies, the directional
 * eta while directions are set.  Per Gauss point, with m_g = w_g rho ca (pi / 4) D_g^2, P = I - a^ a^T and S = [d]x (S x = d x x):
 *     M_g = m_g [  P     -P S  ]
 *               [ S P   -S P S ]
 * in world axes at the body's reference point, with the sign of a mass: the force the member puts on the body is -M (a_lin, alpha),
 * from a_p = a_lin + alpha x d; the centripetal part omega x (omega x d) is left out.  M_g is symmetric and positive semi-definite;
 * a dry segment and a member with ca = 0 contribute exact zeros.  A member's matrix is the serial sum of its points (segment order,
 * the lower point first), a body's the serial sum of its members in index order; the 21 upper entries are computed and mirrored, so
 * M == M^T bitwise, and summing the rows of hc_get_morison_member_added_mass serially in FP64 gives hc_get_morison_added_mass bit
 * for bit.  A body's matrix depends on its pos and rpy, its member list and ca, the wave model with its directions, t, the Morison
 * options and, on the second-order sea, the cut-offs -- not on linvel or angvel, not on other bodies, N or the shard.  The member
 * forces keep their bits whether ca is set or not, and while no owned member has ca > 0 an evaluation launches and allocates nothing
 * more than it did.
 * Not included: point elements (heave-plate added mass normally comes with the BEM data); axial and end-cap added mass; the
 * centripetal term; a frequency-dependent Ca.
 * ca[n] with n the member count of `body` (0-based, any body of the system) as it stands; NULL or n = 0 clears it, and
 * hc_set_morison_members resets the body's ca to 0.  HC_ERR_INVALID: body out of range, n neither 0 nor the member count, a negative
 * or non-finite value, or a hc_morison_begin without its end. */
int hc_set_morison_member_added_mass(hc_ctx* ctx, int body, const double* ca, int n);
int hc_get_morison_member_added_mass_coefficients(hc_ctx* ctx, int body, double* ca_n);
/* The matrix of `body` [6][6] and those of its members [n][6][6] in the last completed evaluation.  HC_ERR_INVALID: a body this
 * context does not own, a null output, or no evaluation with an added-mass part (some owned member with ca > 0) completed since a
 * member list or ca was last set. */
int hc_get_morison_added_mass(hc_ctx* ctx, int body, double* M_6x6);
int hc_get_morison_member_added_mass(hc_ctx* ctx, int body, double* out_nx36);

/* Strip members on the second-order sea (DESIGN.md 3.7c''), long- and short-crested: with `on` (default 0) and
 * hc_set_morison_second_order on, the refusal above is lifted and the members see the increments the elements see -- before the cut
 * and before the drag product.  R, d, P, v_e, the options and the first-order quantities are exactly those of the members above.
 * eta2, u2, a2 are what hc_wave_kinematics2 returns for the same FP64 point and time (hc_wave_kinematics2_dir while wave directions
 * are set), with mwl and regular_phase of the Morison options and the four cut-offs and apply_ramp of hc_set_morison_second_order;
 * everything else of that definition applies as written there (fields held at z2 = min(z - mwl, 0) and at the bed, the true depth,
 * ramp * ramp on all increments).
 *     nodes      h_j = ((P_j.z - mwl) - eta1_j) - eta2_j, in that order of FP64 operations: eta1_j the first-order elevation of the
 *                members above, eta2_j the increment at P_j (1/4 sum ramp^2);  the node is wet iff h_j <= 0
 *     segments, quadrature, weights: unchanged, from the new h
 *     per point  u_f = ramp u1 + u2,  a_f = ramp a1 + a2, with u2 and a2 taken at the point p the cut yields (the y components are 0
 *                in the long-crested sea); stretching stays by the point's own eta1; no second wet test; the force formula is unchanged
 *     dry segments: no pair sum runs at their two points; their increments and their 6-vectors are exact zeros
 * NoWave, no wave model, a record without components or cut-offs that leave no pair inside either band: no further launch, the
 * result is that of order 1 bit for bit.  Both sum levels and the one addition elements + members are unchanged; a body's bits depend
 * on that body's state, its own member list, the wave model with its directions, t, the options and the cut-offs only.  The pair
 * tables are those of hc_set_morison_second_order: elements and members share the one set of the Morison lane.
 * The switch is independent of hc_set_morison_second_order and hc_set_morison_second_order_directional: it keeps its value when
 * they change and has no effect while the first is off.  Two refusals of hc_morison_begin stay and are checked first: wave
 * directions without hc_set_morison_second_order_directional, and more than 4096 components (HC_ERR_UNSUPPORTED, nothing pending).
 * HC_ERR_INVALID: a hc_morison_begin without its end.  on = 0 frees the members' increment buffers (the pair tables are freed by
 * on = 0 of hc_set_morison_second_order).
 * Not included: stretching of the second-order part. */
int hc_set_morison_members_second_order(hc_ctx* ctx, int on);
int hc_get_morison_members_second_order(hc_ctx* ctx, int* on);
/* What the members of `body` (0-based, owned by this context) saw in the last completed evaluation that had a second-order member
 * part, over the body's members in index order: the nodes P[n][3] and eta2[n], n = sum (n_seg + 1); the Gauss points p[n][3] with
 * eta2[n], vel2[n][3], acc2[n][3], n = sum 2 n_seg (segment order, the lower point first; exact zeros behind the point of a dry
 * segment).  The increments are those hc_wave_kinematics2 / hc_wave_kinematics2_dir return for the stored points, bit for bit.  Any
 * pointer may be NULL.  HC_ERR_INVALID: the switch is off, no such evaluation has completed, a member list has changed since, or the
 * body is not owned by this context. */
int hc_get_morison_member_node_increments(hc_ctx* ctx, int body, double* p_nx3, double* eta2_n);
/* The two n of the member list of `body` (any body of the system) as it stands: sum (n_seg + 1) and sum 2 n_seg; either pointer
 * may be NULL.  The two getters refuse after a list change, so these are the sizes of whatever they answer with. */
int hc_get_morison_member_increment_counts(hc_ctx* ctx, int body, int* nodes, int* points);
int hc_get_morison_member_point_increments(hc_ctx* ctx, int body, double* p_nx3, double* eta2, double* vel2_nx3, double* acc2_nx3);

/* ------------------------------------------------------------------------------------------------
 * Nonlinear buoyancy and Froude-Krylov forces on body surface panels (not in the reference: src/hydro_types.h:33 is a TODO): the
 * hydrostatic and incident-wave pressure integrated over the instantaneous wetted surface, an opt-in replacement of the linear
 * hydrostatic term (and, with a scattering-only excitation, of the incident-wave part of the excitation).
 *
 * Panels.  Body b may carry n_b >= 0 panels.  A panel is a centroid c [m] and an area vector s [m^2]: |s| is the area, the
 * direction the outward normal (body into water); both in the body frame, relative to the point pos[b] locates, as a Morison
 * element's r.  Centroid rule, no waterline clipping: a panel is wholly wet or wholly dry by its centroid (the deliberate
 * approximation).
 *
 * Per panel, with pos, rpy of hc_step and the options (mwl, regular phase, stretching) exactly as the Morison term uses them:
 *     R = Rx(rpy0) Ry(rpy1) Rz(rpy2),  d = R c,  p = pos + d,  n = R s
 *     theta_i = k_i p.x - w_i t + phi_i,  eta = sum_i A_i cos theta_i  (expression and component order of hc_wave_kinematics: eta
 *         equals what it returns for that point and time, bit for bit, under the same options)
 *     wet iff p.z - mwl <= eta; a dry panel contributes nothing
 *     p_s = -rho g (p.z - mwl),  g = |gravity|
 *     p_d = rho sum_i (w_i^2 A_i / k_i) px_i(z_e) cos theta_i   (-rho dphi/dt of the potential whose gradient is the velocity of
 *         hc_wave_kinematics); px_i is its x-profile, e^{k z_e} or cosh(k (z_e + d)) / sinh(k d) per component by the reference's
 *         profile test; z_e is exactly what the kinematics take: under Wheeler stretching the stretched z with the reference's second
 *         mwl subtraction, otherwise p.z - mwl; the infinite-depth limit included.  p_s always uses the true p.z.
 *     p_d is multiplied by the ramp the Morison term applies to u_f, under the same conditions (the two synthesised irregular models;
 *         a regular wave is not ramped).  The eta of the wet test is not ramped.
 *     NoWave, no wave model, or an imported eta record (unless components are set): eta = p_d = 0; the kernel still runs and gives
 *     pure nonlinear buoyancy.
 *     buoy_e = (-p_s n, d x (-p_s n)),  fk_e = (-p_d n, d x (-p_d n)): world frame, at the body reference, the sign of an applied force.
 * Per owned body three 6-vectors: buoy and fk, the sums over its panels (a deterministic sum: its bits depend on that body's state,
 * its own panel list, the wave model, t and the options only -- not on the number of bodies, on other bodies' lists, or on the shard
 * context that computes it), and hs_lin, the linear hydrostatic term of hc_step for the same pos, rpy (-rho |g| K_hs dq, the buoyancy
 * force and the (cb - cg) x moment), computed on the host by hc_nonlinear_end so that a caller can replace the linear term without
 * reading step state (hc_get_force_components synchronises the device and has no place in a per-step composition).
 *
 * The terms are NOT part of hc_step & co., hc_get_force_components, hc_compute_* or the Morison calls: a caller composes
 * total - hs_lin + buoy (+ fk) (the HydroForces / TestHydro layers do).  The library subtracts nothing from the wave excitation: when fk
 * is added, the excitation data handed to the context should be the scattering part only.  hc_load_bemio_h5 reads the TOTAL excitation
 * and is not changed.  The path runs on a stream of its own, beside the steps, and touches no step state: hc_nonlinear_begin may be
 * followed by hc_step and then hc_nonlinear_end.  The kinematics assume z up: gravity must be (0, 0, -g).
 * ---------------------------------------------------------------------------------------------- */
typedef struct hc_surface_panel {
    double c[3];
    double s[3];
} hc_surface_panel;
/* Replaces the list of `body` (0-based, any body of the system; a shard context computes those of its own bodies); n = 0 clears
 * it.  Before or after hc_finalize, between evaluations.  HC_ERR_INVALID: body out of range, n < 0, a null list with n > 0, a
 * non-finite value, more than 1048576 panels, or a hc_nonlinear_begin without its end. */
int hc_set_surface_panels(hc_ctx* ctx, int body, const hc_surface_panel* panels, int n);
int hc_get_surface_panel_count(hc_ctx* ctx, int body, int* n);

/* Triangles clipped at the instantaneous free surface: the second kind of surface list, opt-in, without the centroid rule's steps.
 *
 * Triangle lists.  Body b may carry n_b >= 0 triangles v[3][3] [m]: the vertices in the body frame, relative to the point pos[b]
 * locates, counter-clockwise seen from the water (the outward normal is along (v1 - v0) x (v2 - v0)).  Degenerate (zero-area)
 * triangles are allowed.  At most 1048576 triangles per body.  A body carries panels OR triangles: each of the two setters clears
 * the other list of that body.
 *
 * Per vertex j, with pos, rpy and the options of hc_set_nonlinear_options:
 *     R as above,  d_j = R v_j,  P_j = pos + d_j
 *     eta_j, p_s,j, p_d,j: exactly what the panel definition above gives for a panel whose point p is P_j -- the same expressions,
 *         component order, profile test, stretching with the second mwl subtraction, infinite-depth limit and ramp; still water for
 *         NoWave, no model or an eta record (unless components are set).  eta_j equals hc_wave_kinematics at (P_j, t), bit for bit, under the same options.
 *     h_j = P_j.z - mwl - eta_j; the vertex is wet iff h_j <= 0.
 * Wet part.  h, p_s and p_d are taken as linear over the triangle; the wet part is {h <= 0}:
 *     0 wet vertices   nothing
 *     3 wet vertices   the whole triangle
 *     1 wet vertex a, with b, c following in cyclic order:          the sub-triangle (a, ab, ac)
 *     2 wet vertices, dry vertex c, a, b following c cyclically:    the sub-triangles (a, b, bc) and (a, bc, ca)
 *     xy is the point of edge x -> y at s = h_x / (h_x - h_y), x being the WET end: h_x <= 0 < h_y, the denominator is never zero;
 *     d, p_s and p_d at xy are interpolated with that same s.
 * Per sub-triangle (q0, q1, q2): S = 1/2 (q1 - q0) x (q2 - q0); at the three edge midpoints m the pressure p_m is the mean of the two
 * end values; F = sum_m (-p_m S / 3), M = sum_m m x (-p_m S / 3): exact for a pressure linear in space, the moment included.  buoy
 * takes p_s, fk takes p_d: world frame, at the body reference, the sign of an applied force.  A body's buoy and fk are the sums over
 * its triangles, deterministic as above: the bits depend on that body's state, its own list, the wave model, t and the options
 * only -- not on the number of bodies, on other bodies' lists of either kind, or on the shard.  hs_lin is unchanged.
 *
 * Consequences.  In still water buoy is the exact hydrostatic force and moment of the polyhedron below the plane, at any attitude
 * and draft, with any mesh, and it is continuous in the state.  In waves the free surface is linearised per triangle: second order
 * in the triangle size.  The p_d of a vertex above the wave is the extrapolated profile (the centroid rule already uses the
 * extrapolated profile above the mean level).
 *
 * HC_ERR_INVALID as hc_set_surface_panels: body out of range, n < 0, a null list with n > 0, a non-finite value, more than 1048576
 * triangles, or a hc_nonlinear_begin without its end.  n = 0 clears the list. */
int hc_set_surface_triangles(hc_ctx* ctx, int body, const double* tri /* [n][3][3] */, int n);
int hc_get_surface_triangle_count(hc_ctx* ctx, int body, int* n);
/* mwl, regular_phase, wave_stretching of the kinematics the panels and triangle vertices see; NULL = the defaults */
int hc_set_nonlinear_options(hc_ctx* ctx, const hc_wave_kinematics_opts* o);
/* begin enqueues (pos, rpy as for hc_step: [3N] each), end waits and copies the 6 * n_local values of each of the three terms (any
 * output pointer may be NULL); exactly one end per begin.  Needs hc_finalize.  HC_ERR_INVALID on a non-finite state or t, on a
 * gravity that is not (0, 0, -g), on a second begin, on an end without a begin; nothing stays pending after a failure.  Panels and
 * triangles are served by one evaluation.  With no panel and no triangle on any owned body: buoy = fk = 0, no launch. */
int hc_nonlinear_begin(hc_ctx* ctx, double t, const double* pos, const double* rpy);
int hc_nonlinear_end(hc_ctx* ctx, double* buoy_Dlocal, double* fk_Dlocal, double* hs_lin_Dlocal);
int hc_compute_nonlinear(hc_ctx* ctx, double t, const double* pos, const double* rpy, double* buoy_Dlocal, double* fk_Dlocal,
                         double* hs_lin_Dlocal);

/* The surface on the second-order sea: with `on` the panels and the clipped triangles see Sharma and Dean's
 * long-crested sea to second order -- the wetted surface ends at eta1 + eta2 and the pressure is Bernoulli's to second order.  A
 * surface point is a panel's centroid or a triangle's vertex; its world position P = pos + R c is the FP64 expression above.  At
 * every surface point:
 *     eta2 = hc_wave_kinematics2 (below) at the same FP64 point P and time t, with mwl and regular_phase of the nonlinear options
 *         (hc_set_nonlinear_options) and the four cut-offs [rad/s] and apply_ramp of this call -- bit for bit that call's value
 *     q2   = -d phi2 / dt = sum_{+-} sum_i sum_j B+-_ij Omega C(kappa, z2) cos Theta  [m^2/s^2], of that definition's
 *         phi2 = sum B C sin Theta: the same pair tables, bands, profile C, z2 = min(P.z - mwl, 0) held at the bed, and the signs of
 *         kappa, Omega, Theta of u2x; times ramp * ramp with apply_ramp, as the other increments
 *     u1   = (u1x, u1z), the first-order velocity of hc_wave_kinematics at P, at the z_e p_d is taken at (stretching by eta1 with
 *         the second mwl subtraction, the reference's profile test); not ramped
 *     panels:    wet iff P.z - mwl <= eta1 + eta2
 *     triangles: h_j = P_j.z - mwl - (eta1_j + eta2_j)
 *     p_s unchanged;   p_d = ramp p_d1 + rho q2 - 1/2 rho ramp^2 (u1x^2 + u1z^2),  p_d1 and ramp those of order 1 (ramp = 1 where
 *         order 1 applies none)
 * and everything after that -- the case table, the midpoint rule, the split into buoy and fk, hs_lin -- is unchanged.  The two added
 * terms are what cancels the first-order pressure's second-order residue at the free surface: p_s + p_d at z = mwl + eta1 + eta2 is
 * of third order in the amplitudes.  They enter before the wet test and the clipping, so the result cannot be composed from the
 * other calls.
 * NoWave, no wave model, an imported eta record (unless components are set), or cut-offs that leave no pair inside either band: the launches and the bits of
 * order 1.  With on = 0 (the default) every call makes the launches and returns the bits it did before this switch existed.  A
 * body's bits still depend on that body's state and list, the wave model, t and the options only.
 * The pair tables are this path's own (a third copy of 4 nf^2 doubles beside those of hc_wave_kinematics2 and the Morison
 * elements: 8 MB at 512 components, 537 MB at 4096), built on its stream, cached on the wave model, the regular phase and the
 * cut-offs and freed by on = 0 with the point and increment buffers.  The pair sum runs once per DISTINCT body-frame point of a
 * body's list (two points are the same when their three doubles have equal bits): a closed mesh costs about half a point per
 * triangle.  HC_ERR_INVALID: a negative or NaN cut-off, lo > hi, or a hc_nonlinear_begin without its end.  More than 4096 wave
 * components: hc_nonlinear_begin returns HC_ERR_UNSUPPORTED and nothing stays pending.
 * Not included: second order in the drift term (which keeps seeing the first-order sea), stretching of the second-order part, a
 * bound on the extrapolated first-order pressure at dry vertices. */
int hc_set_nonlinear_second_order(hc_ctx* ctx, int on, double diff_lo, double diff_hi, double sum_lo, double sum_hi, int apply_ramp);
int hc_get_nonlinear_second_order(hc_ctx* ctx, int* on, double* diff_lo, double* diff_hi, double* sum_lo, double* sum_hi, int* apply_ramp);
/* The same in a short-crested sea.  While hc_set_nonlinear_second_order is on and wave directions are set
 * (hc_set_wave_directions; a uniform heading on the IRF model and a regular wave with one heading included), hc_nonlinear_begin
 * answers HC_ERR_UNSUPPORTED unless this switch is on (default 0).  With it on, every surface point P sees
 *     eta  = eta1 + eta2 in the wet test and the clipping height: eta1 of the directional first-order kernels, eta2 what
 *         hc_wave_kinematics2_dir returns for the same FP64 point P and time, bit for bit, with mwl and regular_phase of the
 *         nonlinear options and the four cut-offs and apply_ramp of hc_set_nonlinear_second_order
 *     q2   = -d phi2 / dt = sum_{+-} sum_ij B+-_ij Omega+-_ij C(|kappa+-_ij|, z2) cos Theta+-_ij, times ramp * ramp: the pair tables,
 *         bands, weights, z2, |kappa| = |k_i e_i +- k_j e_j| and profile C of that call's u2x
 *     u1   = (u1x, u1y, u1z), the unramped first-order directional velocity at the z_e of p_d1; its horizontal part lies along
 *         every component's direction
 *     p_d  = ramp p_d1 + rho q2 - 1/2 rho ramp^2 (u1x^2 + u1y^2 + u1z^2)
 * and everything else as above.  The pair tables are those of the directional pair sum, again this path's own (the one set of this
 * path holds either kind, rebuilt when the directions come or go); on = 0 of hc_set_nonlinear_second_order frees them.  The rules
 * above carry over: no components or no pair inside either band -- no second-order launch and the directional first-order bits; more
 * than 4096 components -- HC_ERR_UNSUPPORTED from hc_nonlinear_begin; hc_get_nonlinear_increments answers as before.
 * The switch is independent of hc_set_nonlinear_second_order: it keeps its value when that one goes off and on, has no effect while
 * that one is off, and none without directions (the long-crested path, its kernels and its bits).  HC_ERR_INVALID: a
 * hc_nonlinear_begin without its end.  `on` of the getter may be NULL. */
int hc_set_nonlinear_second_order_directional(hc_ctx* ctx, int on);
int hc_get_nonlinear_second_order_directional(hc_ctx* ctx, int* on);
/* The number of distinct surface points of `body` (0-based, any body of the system): of its panel centroids or its triangle
 * vertices, in the order of their first use. */
int hc_get_nonlinear_point_count(hc_ctx* ctx, int body, int* n);
/* What the surface points of `body` (0-based, owned by this context) saw in the last completed evaluation that had a second-order
 * part: their world positions p[n][3] and eta2[n], q2[n]; n = the body's point count at that evaluation.  Any pointer may be NULL.
 * Also answered between a later hc_nonlinear_begin and its end.  HC_ERR_INVALID: the switch is off, no such evaluation has
 * completed (one without a second-order part forgets the one before, and so do hc_set_surface_panels / _triangles), n is not
 * the point count, or the body is not owned by this context. */
int hc_get_nonlinear_increments(hc_ctx* ctx, int body, int n, double* p /* [n][3] */, double* eta2 /* [n] */, double* q2 /* [n] */);

/* ------------------------------------------------------------------------------------------------
 * Second-order wave drift forces from difference-frequency QTF tables (not in the reference, whose wave forces are first order in
 * the amplitude: no mean, no energy below the wave band).  Opt-in, per body, evaluated at the body's instantaneous position.
 *
 * Data per body: a frequency grid Omega[0..nq) [rad/s], finite and strictly increasing, 2 <= nq <= 256, and P[6][nq][nq],
 * Q[6][nq][nq] (row-major): real and imaginary part of the difference-frequency QTF T_d(Omega_m, Omega_n) of the six body rows, in
 * force (moment) per squared wave amplitude, already dimensional -- the library applies no rho or g.  Q may be NULL (zeros).  No
 * Hermitian symmetry is required or enforced.
 *
 * Components (A_i, w_i, k_i, phi_i): those of the context's wave model, exactly as hc_wave_kinematics sees them (a regular wave: one
 * component with the regular_phase option).  For body b, theta_i = k_i pos[b].x - w_i t + phi_i in that kernel's expression; only x
 * enters (the reference's long-crested waves along +x); rotation, y, z, mwl and stretching do not.
 *
 * Interpolation: a component with w_i < Omega_0 or w_i > Omega_{nq-1} takes no part, in any mode.  Otherwise m_i is the largest m
 * with Omega_m <= w_i, capped at nq - 2, lambda_i = (w_i - Omega_m) / (Omega_{m+1} - Omega_m), W[i][m_i] = 1 - lambda_i,
 * W[i][m_i + 1] = lambda_i, 0 elsewhere; both ends of the grid are inside.  D_d(w) is the diagonal P_d[m][m] interpolated with W.
 *
 * Modes (hc_set_drift_mode; 0 = off, the default):
 *     1  mean drift           F_d = sum_i A_i^2 D_d(w_i)
 *     2  Newman               F_d = sum_i sum_j A_i A_j 1/2 (D_d(w_i) + D_d(w_j)) cos(theta_i - theta_j)
 *     3  full QTF             F_d = sum_i sum_j A_i A_j [P_d(w_i, w_j) cos(theta_i - theta_j) - Q_d(w_i, w_j) sin(theta_i - theta_j)],
 *                             P_d(w_i, w_j) = sum_mn W[i][m] W[j][n] P_d[m][n] (bilinear), Q likewise
 * Modes 1 and 2 read the diagonal of P only.  Mode 3 on a table that holds a diagonal only (mean-drift coefficients) is the caller's
 * mistake: the zeros off the diagonal are taken as data.
 * The result is multiplied by ramp * ramp (second order in the amplitude), ramp being the factor the Morison term applies to u_f
 * under the same conditions: the two synthesised irregular models are ramped, a regular wave is not.
 * NoWave, no wave model, an imported eta record (no components, unless components are set), mode 0: zeros, no launch.  A body without a table: zeros.
 * World frame, at the body reference, the sign of an applied force.  A regular wave gives the constant A^2 T(w, w).
 * Sum-frequency QTFs are a term of their own (hc_set_sum_qtf below).  The tables hold one heading: while wave directions are set
 * (hc_set_wave_directions) and some body holds such a table hc_drift_begin with a mode != 0 returns HC_ERR_UNSUPPORTED.
 *
 * QTF tables on a heading grid (hc_set_drift_qtf_headings, hc_set_sum_qtf_headings; both terms): what is evaluated while directions
 * are set.  Per body and term a heading grid beta[0..nh) [rad], world frame, 0 along +x as hc_set_wave_directions, finite and
 * strictly increasing, 1 <= nh <= 16, the frequency grid Omega[0..nq) as above, J = nh nq <= 1024, and P, Q [6][nh][nh][nq][nq]
 * (row-major, Q may be NULL): element (d, a, b, m, n) is T(beta_a, beta_b, Omega_m, Omega_n), a and m belonging to component i of a
 * pair, b and n to component j.  Dimensional; no symmetry is required or enforced.  A body holds one table per term: either setter
 * replaces what the other stored; nq = 0 clears.
 * Phase: that of the directional kinematics, psi_i = k_i (x cos theta_i + y sin theta_i) - w_i t + phi_i with x, y = pos[b]; with no
 * directions set every theta_i = 0, the theta_i of the one-heading tables.  Frequency weights: exactly those above.  Heading weights:
 * a_i is the largest a with beta_a <= theta_i, mu_i = (theta_i - beta_a) / (beta_{a+1} - beta_a), Wh[i][a_i] = 1 - mu_i,
 * Wh[i][a_i + 1] = mu_i; a theta on a node has weight exactly 0 on the neighbour; nh = 1 is valid for theta_i == beta_0 only; no
 * extrapolation and no wrap-around.  A component inside the frequency grid whose theta_i lies outside [beta_0, beta_{nh-1}] makes
 * the begin call fail with HC_ERR_INVALID, nothing pending (it is not dropped silently).  The body's yaw is NOT applied to the
 * headings, as with the first-order heading tables.
 * With the node weight w_i,(a,m) = Wh[i][a] Wf[i][m], T(i, j) = sum_{a,b,m,n} w_i,(a,m) w_j,(b,n) T[a][b][m][n] and
 * D(i) = sum_{a,m} w_i,(a,m) P[a][a][m][m] take the places of P_d(w_i, w_j), Q_d(w_i, w_j) and D_d(w_i) in the modes above and in the
 * sum-frequency term, with psi for theta; ramp^2, the zero cases, the frame and the sign are unchanged.  The device evaluates the
 * same projected form over the nodes p = a nq + m, O(nf + J^2) per row, in a fixed order: a body's bits depend on its own table,
 * pos[b].x, pos[b].y, t, the wave model with its directions, the mode and the regular phase only.
 *
 * The device evaluates the exact projected form, O(nf + nq^2) per row: with u_i = A_i cos theta_i, w_i = A_i sin theta_i,
 * U_m = sum_i W[i][m] u_i, V_m = sum_i W[i][m] w_i,
 *     mode 3  F_d = sum_mn P_d[m][n] (U_m U_n + V_m V_n) - Q_d[m][n] (V_m U_n - U_m V_n)
 *     mode 2  F_d = (sum_m D_m U_m)(sum_m U_m) + (sum_m D_m V_m)(sum_m V_m)
 *     mode 1  F_d = sum_m D_m E_m,  E_m = sum_i W[i][m] A_i^2
 * in a fixed order: a body's bits depend on its own table, pos[b].x, t, the wave model, the mode and the regular phase only -- not
 * on the number of bodies, on other bodies' tables, or on the shard context that computes it.
 *
 * The term is NOT part of hc_step & co., hc_get_force_components, hc_compute_* or the Morison and nonlinear calls; a caller adds it
 * (the HydroForces / TestHydro layers do).  The path runs on a stream of its own, beside the steps, and touches no step state, no
 * history and no per-time cache: hc_drift_begin may be followed by hc_step and then hc_drift_end.
 * ---------------------------------------------------------------------------------------------- */
/* Replaces the table of `body` (0-based, any body of the system; a shard context computes those of its own bodies); nq = 0 clears
 * it.  Before or after hc_finalize, between evaluations.  HC_ERR_INVALID: body out of range, nq of 1, negative or above 256, a null
 * grid or P with nq > 0, a non-finite value, a grid that is not strictly increasing, or a hc_drift_begin without its end. */
int hc_set_drift_qtf(hc_ctx* ctx, int body, int nq, const double* omega, const double* P, const double* Q);
int hc_get_drift_qtf_size(hc_ctx* ctx, int body, int* nq);
/* The same on a heading grid ("QTF tables on a heading grid" above): replaces the table of `body`, of either kind; nq = 0 clears it.
 * HC_ERR_INVALID in addition: nh outside 1 .. 16, nh nq above 1024, a null, non-finite or not strictly increasing heading grid.
 * *nh of the getter: 0 for a one-heading table or none.  hc_get_drift_qtf_size reports nq for both kinds. */
int hc_set_drift_qtf_headings(hc_ctx* ctx, int body, int nh, const double* beta, int nq, const double* omega, const double* P, const double* Q);
int hc_get_drift_qtf_headings(hc_ctx* ctx, int body, int* nh);
/* 0 off (default), 1 mean drift, 2 Newman's approximation, 3 full QTF; HC_ERR_INVALID outside 0..3 or while a begin is pending */
int hc_set_drift_mode(hc_ctx* ctx, int mode);
int hc_get_drift_mode(hc_ctx* ctx, int* mode);
/* only regular_phase is read; NULL = the defaults */
int hc_set_drift_options(hc_ctx* ctx, const hc_wave_kinematics_opts* o);
/* begin enqueues (pos as for hc_step: [3N]), end waits and copies the 6 * n_local values; exactly one end per begin.  Needs
 * hc_finalize.  HC_ERR_INVALID on a non-finite t or pos, on a second begin, on an end without a begin; nothing stays pending after a
 * failure. */
int hc_drift_begin(hc_ctx* ctx, double t, const double* pos);
int hc_drift_end(hc_ctx* ctx, double* out_Dlocal);
int hc_compute_drift(hc_ctx* ctx, double t, const double* pos, double* out_Dlocal);

/* ------------------------------------------------------------------------------------------------
 * Second-order wave forces from sum-frequency QTF tables (not in the reference): the other output of a second-order diffraction
 * run, the excitation above the wave band (springing and ringing of tendons, heave and pitch of stiff platforms).  Opt-in, per
 * body, evaluated at the body's instantaneous position; independent of the drift term above (tables, grid, mode and options of its
 * own).
 *
 * Data per body: a frequency grid Omega[0..nq) [rad/s] of its own, finite and strictly increasing, 2 <= nq <= 256, and
 * P[6][nq][nq], Q[6][nq][nq] (row-major): real and imaginary part of the sum-frequency QTF T_s(Omega_m, Omega_n) of the six body
 * rows, in force (moment) per squared wave amplitude, already dimensional.  Q may be NULL (zeros).  No symmetry is required or
 * enforced; since cos and sin of theta_i + theta_j are symmetric in (i, j), only the symmetric part 1/2 (T_s[m][n] + T_s[n][m]) of a
 * table can contribute, and a purely antisymmetric table gives zero.
 *
 * Components, theta_i, the inside test, the cell m_i, lambda_i and the weights W[i][m]: those of the drift term, word for word (both
 * grid ends inside).
 *
 *     F_s = ramp^2 sum_i sum_j A_i A_j [P_s(w_i, w_j) cos(theta_i + theta_j) - Q_s(w_i, w_j) sin(theta_i + theta_j)],
 *     P_s(w_i, w_j) = sum_mn W[i][m] W[j][n] P_s[m][n] (bilinear), Q likewise,
 * i.e. Re sum_ij A_i A_j T_s(w_i, w_j) exp(i (theta_i + theta_j)).  ramp as for the drift term: the two synthesised irregular models
 * are ramped, a regular wave is not; a regular wave gives A^2 [P_s(w, w) cos 2 theta - Q_s(w, w) sin 2 theta].
 * NoWave, no wave model, an imported eta record (no components, unless components are set), mode 0: zeros, no launch.  A body without a table: zeros.
 * World frame, at the body reference, the sign of an applied force.
 * There is no cut-off band on w_i + w_j: a caller who wants one zeroes table entries.  The tables hold one heading: while wave
 * directions are set (hc_set_wave_directions) and some body holds such a table hc_sum_qtf_begin with a mode != 0 returns
 * HC_ERR_UNSUPPORTED; tables on a heading grid (hc_set_sum_qtf_headings, defined with the drift term above) are evaluated.
 *
 * The device evaluates the exact projected form, O(nf + nq^2) per row, with the U_m, V_m of the drift term:
 *     F_s = sum_mn P_s[m][n] (U_m U_n - V_m V_n) - Q_s[m][n] (V_m U_n + U_m V_n)
 * in a fixed order: a body's bits depend on its own table, pos[b].x, t, the wave model and the regular phase only -- not on the
 * number of bodies, on other bodies' tables, or on the shard context that computes it.
 *
 * The term is NOT part of hc_step & co., hc_get_force_components, hc_compute_* or the Morison, nonlinear and drift calls; a caller
 * adds it (the HydroForces / TestHydro layers do, after the drift term).  The path runs on a stream of its own, beside the steps,
 * and touches no step state: hc_sum_qtf_begin may be followed by hc_step and then hc_sum_qtf_end.
 * ---------------------------------------------------------------------------------------------- */
/* As hc_set_drift_qtf: replaces the table of `body` (0-based, any body of the system); nq = 0 clears it.  HC_ERR_INVALID: body out
 * of range, nq of 1, negative or above 256, a null grid or P with nq > 0, a non-finite value, a grid that is not strictly
 * increasing, or a hc_sum_qtf_begin without its end. */
int hc_set_sum_qtf(hc_ctx* ctx, int body, int nq, const double* omega, const double* P, const double* Q);
int hc_get_sum_qtf_size(hc_ctx* ctx, int body, int* nq);
/* As hc_set_drift_qtf_headings / hc_get_drift_qtf_headings, for the sum-frequency table of `body` */
int hc_set_sum_qtf_headings(hc_ctx* ctx, int body, int nh, const double* beta, int nq, const double* omega, const double* P, const double* Q);
int hc_get_sum_qtf_headings(hc_ctx* ctx, int body, int* nh);
/* 0 off (default), 1 on; HC_ERR_INVALID otherwise or while a begin is pending */
int hc_set_sum_mode(hc_ctx* ctx, int mode);
int hc_get_sum_mode(hc_ctx* ctx, int* mode);
/* only regular_phase is read; NULL = the defaults */
int hc_set_sum_options(hc_ctx* ctx, const hc_wave_kinematics_opts* o);
/* begin enqueues (pos as for hc_step: [3N]), end waits and copies the 6 * n_local values; exactly one end per begin.  Needs
 * hc_finalize.  HC_ERR_INVALID on a non-finite t or pos, on a second begin, on an end without a begin; nothing stays pending after a
 * failure. */
int hc_sum_qtf_begin(hc_ctx* ctx, double t, const double* pos);
int hc_sum_qtf_end(hc_ctx* ctx, double* out_Dlocal);
int hc_compute_sum_qtf(hc_ctx* ctx, double t, const double* pos, double* out_Dlocal);

/* ------------------------------------------------------------------------------------------------
 * Second-order irregular waves (not in the reference): the second-order increments of the long-crested sea of Sharma and Dean
 * (1981) to the elevation, velocity and acceleration of hc_wave_kinematics, batched over points x times, on the GPU.  The caller
 * adds them to the first-order values.  DESIGN.md 3.7f has the derivation checks and the kernels.
 *
 * Components (A_i, w_i, k_i, phi_i), i < nf: those of the context's wave model, exactly as hc_wave_kinematics sees them (a regular
 * wave: one component with the regular_phase option); theta_i = k_i x - w_i t + phi_i in that kernel's expression; g = |g| and
 * h = the water depth of the context.  h may be infinite (tanh -> 1, the profiles become e^{kappa z}).  The reference's
 * "exponential profile when 2 pi / k > depth" test is deliberately NOT applied here: the second-order terms always use the true
 * depth (the first-order part stays the reference's).
 *     R_i = w_i^2 / g (from w, not from k tanh k h: the reference's k is on the dispersion curve to 1e-6 only),
 *     r_i = sqrt(R_i),  b_i = A_i g / w_i
 * For a pair (i, j) and a sign +-:  kappa = k_i +- k_j (signed),  Omega = w_i +- w_j,  Theta = theta_i +- theta_j,
 * T(kappa) = |kappa| tanh(|kappa| h),
 *     den+-  = (r_i +- r_j)^2 - T(kappa)
 *     D+_ij  = [ (r_i + r_j) (r_i (k_j^2 - R_j^2) + r_j (k_i^2 - R_i^2)) + 2 (r_i + r_j)^2 (k_i k_j - R_i R_j) ] / den+
 *     D-_ij  = [ (r_i - r_j) (r_j (k_i^2 - R_i^2) - r_i (k_j^2 - R_j^2)) + 2 (r_i - r_j)^2 (k_i k_j + R_i R_j) ] / den-
 *     K+-_ij = (D+-_ij - (k_i k_j -+ R_i R_j)) / (r_i r_j) + (R_i + R_j)
 *     B+-_ij = 1/4 b_i b_j D+-_ij / Omega,                 D-_ij = B-_ij = 0 where w_i == w_j
 * With C(kappa, z) = cosh(|kappa| (z + h)) / cosh(|kappa| h), S likewise with sinh in the numerator (both e^{|kappa| z} for an
 * infinite h), all sums over every i, every j and, where B appears, both signs:
 *     eta2 = 1/4 sum A_i A_j [K-_ij cos(theta_i - theta_j) + K+_ij cos(theta_i + theta_j)]
 *     u2x  = sum B kappa C cos Theta          u2z = sum B |kappa| S sin Theta            (y components 0)
 *     a2x  = sum B kappa Omega C sin Theta    a2z = -sum B |kappa| Omega S cos Theta     (local acceleration, as first order)
 * (the gradient and its time derivative of phi2 = sum B C sin Theta).  The profiles are taken at z2 = min(z - mwl, 0), and at -h
 * below the bed: above the mean level the second-order fields are held at their mean-level value (the expansion is about z = 0;
 * e^{(k_i + k_j) z} is not extrapolated upward).  No Wheeler stretching applies to these terms.
 *
 * Cut-offs [rad/s]: a difference term takes part when diff_lo <= |w_i - w_j| <= diff_hi, a sum term when sum_lo <= w_i + w_j <=
 * sum_hi; the defaults 0 and +inf take everything.  They decide the cost: only the band of the pair matrix is visited, a band
 * that excludes every pair of a sign skips that sign, and two empty bands give zeros without a launch.
 * Ramp: with apply_ramp (the default) the increments are multiplied by ramp * ramp, ramp being the factor the Morison term applies
 * to u_f under the same conditions (the two synthesised irregular models, ramp_duration > 0 and t < ramp_duration; a regular wave
 * is not ramped).  hc_wave_kinematics itself is not ramped, hence the switch.
 * NoWave, no wave model, or an imported eta record (no components, unless components are set): zeros, no launch.  A regular wave: the single pair i = j,
 * which is Stokes' second-order term plus the constant set-down.  More than 4096 components: HC_ERR_UNSUPPORTED (the four pair
 * tables take 4 nf^2 doubles of device memory: 8 MB at 512 components, 134 MB at 2048, 537 MB at 4096).
 *
 * Every (point, time) item is summed by one workgroup in a fixed order: its bits depend on the item, the wave model and the
 * options only -- not on the batch it is part of, its place in it, the outputs asked for, or the shard context that answers.
 * The drift term keeps seeing the first-order field; the Morison elements and the surface panels and triangles see these
 * increments once hc_set_morison_second_order / hc_set_nonlinear_second_order switch them on.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hc_wave_kinematics2_opts {
    double mwl;            /* WaveBase::mwl_ (0) */
    double regular_phase;  /* RegularWave::regular_wave_phase_ (0) */
    double diff_lo, diff_hi, sum_lo, sum_hi; /* cut-offs in rad/s (0, +inf, 0, +inf) */
    int apply_ramp;        /* (1) */
} hc_wave_kinematics2_opts;
void hc_wave_kinematics2_opts_default(hc_wave_kinematics2_opts* o);
/* xyz[n_points][3], t[n_times] -> eta2[T][P], vel2[T][P][3], acc2[T][P][3]: the contract of hc_wave_kinematics (any output may be
 * NULL, o NULL = the defaults, counts >= 0, a pointer where its count is > 0, finite x, z, t, mwl and regular_phase, at most
 * 2^31 - 256 (point, time) pairs, needs hc_finalize, synchronous, changes no force and no step state; it runs on a stream of its
 * own).  Also HC_ERR_INVALID: a negative or NaN cut-off, or lo > hi. */
int hc_wave_kinematics2(hc_ctx* ctx, const hc_wave_kinematics2_opts* o, int n_points, const double* xyz,
                        int n_times, const double* t, double* eta2, double* vel2, double* acc2);
/* The device's own pair tables K+, K-, B+, B- copied back, [nf][nf] each (row i, column j; nf from hc_get_sizes, 1 for a regular
 * wave); entries outside their cut-off band are 0.  Any pointer may be NULL.  No components: nothing is written. */
int hc_wave_kinematics2_pair_tables(hc_ctx* ctx, const hc_wave_kinematics2_opts* o, double* Kp, double* Km, double* Bp, double* Bm);

/* ------------------------------------------------------------------------------------------------
 * Second-order irregular waves in a short-crested sea (not in the reference): the increments above for components that travel in
 * directions of their own (hc_set_wave_directions).  A call beside hc_wave_kinematics2, which keeps refusing while directions are
 * set.  DESIGN.md 3.7n has the checks and the kernels.
 *
 * Components (A_i, w_i, k_i, phi_i) as above; beta_i the direction of component i and (c_i, s_i) = (cos beta_i, sin beta_i) as the
 * directional first-order kinematics hold them; with no directions set c_i = 1, s_i = 0.  R, r, b as above.
 *     theta_i = k_i (x c_i + y s_i) - w_i t + phi_i                     (the expression of the directional hc_wave_kinematics)
 *     gamma_ij = cos(beta_i - beta_j),   k_i . k_j = k_i k_j gamma_ij
 *     kappa+-_x = k_i c_i +- k_j c_j,  kappa+-_y = k_i s_i +- k_j s_j,  |kappa+-| = sqrt(k_i^2 + k_j^2 +- 2 k_i k_j gamma_ij)
 *     T(kappa) = |kappa| tanh(|kappa| h),   den+- = (r_i +- r_j)^2 - T(kappa+-)
 *     D+_ij  = [ (r_i + r_j) (r_i (k_j^2 - R_j^2) + r_j (k_i^2 - R_i^2)) + 2 (r_i + r_j)^2 (k_i . k_j - R_i R_j) ] / den+
 *     D-_ij  = [ (r_i - r_j) (r_j (k_i^2 - R_i^2) - r_i (k_j^2 - R_j^2)) + 2 (r_i - r_j)^2 (k_i . k_j + R_i R_j) ] / den-
 *     K+-_ij = (D+-_ij - (k_i . k_j -+ R_i R_j)) / (r_i r_j) + (R_i + R_j)
 *     B+-_ij = 1/4 b_i b_j D+-_ij / (w_i +- w_j),          D-_ij = B-_ij = 0 where w_i == w_j
 *     eta2 = 1/4 sum A_i A_j [K-_ij cos(theta_i - theta_j) + K+_ij cos(theta_i + theta_j)]
 *     u2x  = sum B kappa_x C cos Theta        u2y = sum B kappa_y C cos Theta        u2z = sum B |kappa| S sin Theta
 *     a2x  = sum B kappa_x Omega C sin Theta  a2y = sum B kappa_y Omega C sin Theta  a2z = -sum B |kappa| Omega S cos Theta
 * C and S as above at |kappa+-|; the sums over every i, every j and both signs.  In an infinite depth the sum-frequency potential,
 * zero for a long-crested sea, is not zero for two components that cross.  z2, the bed, no stretching, the cut-off bands (on the
 * frequencies alone), ramp * ramp, the 4096-component limit, the zero cases and the regular wave (the single pair i = j, along its
 * heading) are those of hc_wave_kinematics2, and so is the statement on an item's bits.
 *
 * Works with or without directions set: without them it is the long-crested sea along +x evaluated by the directional kernels,
 * equal to hc_wave_kinematics2 to rounding, not bit for bit.  Non-uniform directions exist on the spectral model and a regular wave
 * only; a uniform heading on the IRF model is accepted.  The contract is that of hc_wave_kinematics2 with y finite as well; the
 * tables (a set of this call's own, 4 nf^2 doubles) are cached on the wave model with its directions, the regular phase and the
 * four cut-offs.  The Morison and nonlinear second-order switches keep refusing while directions are set.
 * ---------------------------------------------------------------------------------------------- */
int hc_wave_kinematics2_dir(hc_ctx* ctx, const hc_wave_kinematics2_opts* o, int n_points, const double* xyz,
                            int n_times, const double* t, double* eta2, double* vel2, double* acc2);
int hc_wave_kinematics2_dir_pair_tables(hc_ctx* ctx, const hc_wave_kinematics2_opts* o, double* Kp, double* Km, double* Bp, double* Bm);

/* ------------------------------------------------------------------------------------------------
 * State-space radiation by modal recursion (not in the reference, which carries radiation_calculation: state_space in hydro.yaml
 * and reads no state-space data): the radiation force from a modal model of the impulse response instead of the convolution over
 * the velocity history.  No history and no time grid: the state moves from one accepted time to the next by a closed formula that
 * holds for any step length.  DESIGN.md 3.7r has the mathematics, the kernel and the checks.
 *
 * A mode belongs to a pair (row of an owned body, column c in 0 .. D-1) and has a complex pole lambda, Re lambda < 0, and a complex
 * residue rho:   K_rc(tau) = sum_m Re[rho_m exp(lambda_m tau)].  A real pole has lambda_im = 0; a conjugate pair is ONE mode with the
 * real part taken, its residue twice the pair's.  Residues are in the units of the K given to hc_set_rirf (BEMIO-normalised): the
 * library multiplies them by rho as it does K, so modes fitted to that K give the force the convolution gives.
 *
 * With the velocity linear between two consecutive accepted times t_n < t_n+1, h = t_n+1 - t_n, x = lambda h:
 *     z_n+1 = e^x z_n + h [(phi1(x) - phi2(x)) v_n + phi2(x) v_n+1],   phi1 = (e^x - 1) / x,   phi2 = (e^x - 1 - x) / x^2
 *     rad_r(t_n+1) = sum_c sum_m Re[rho_m z_m]
 * with the sign and meaning of hc_compute_radiation (the total is hs - rad + waves).  The first call, at t_0, sets z = 0, stores
 * v(t_0) and returns zeros.  The term is independent of the convolution: hc_step and hc_compute_radiation are not touched, and a
 * caller subtracts what it has set -- a modes-only caller passes a short zero IRF to hc_set_rirf (hc_finalize still wants one).
 *
 * Time: the lane keeps z and v of the last `depth` accepted times (hc_set_radiation_modes_depth, 2 .. 64, default 4; depth * 16 B
 * per mode).  A call at t above the newest time advances from the newest snapshot.  A call at t equal to it is the convolution's
 * duplicate-time error (HC_ERR_RUNTIME).  A call at t below it is a rejected step: the snapshots at times >= t are dropped and the
 * step advances from the newest one that survives; if none does: HC_ERR_INVALID, the state stays as it was.
 *
 * It runs on a stream of its own beside the steps, as the Morison term does: hc_radiation_modes_begin copies the velocities up and
 * enqueues, hc_radiation_modes_end waits and copies out; exactly one end per begin.  A row's bits depend on that row's modes, the
 * velocity samples and the times only -- not on N, on other rows' lists or on the shard.  Not part of hc_step_device / hc_step_multi.
 * ---------------------------------------------------------------------------------------------- */
typedef struct hc_radiation_mode {
    int row; /* 0 .. 5 of the body */
    int col; /* 0 .. D-1 */
    double lambda_re, lambda_im, rho_re, rho_im;
} hc_radiation_mode;
/* Replaces the list of `body` (0-based, any body of the system; one outside this context's shard is accepted and ignored); n = 0
 * clears it.  Within a pair the modes keep the order given.  A changed list empties the snapshot ring: the next call is a first
 * call.  HC_ERR_INVALID: body out of range, n < 0, a null list with n > 0, a non-finite value, Re lambda >= 0, a row or column out
 * of range, more than 16 modes on one pair, or a hc_radiation_modes_begin without its end. */
int hc_set_radiation_modes(hc_ctx* ctx, int body, const hc_radiation_mode* modes, int n);
int hc_get_radiation_mode_count(hc_ctx* ctx, int body, int* n);
/* 2 .. 64 (default 4); empties the ring.  HC_ERR_INVALID outside that range or while a begin is pending. */
int hc_set_radiation_modes_depth(hc_ctx* ctx, int depth);
/* linvel, angvel [3N] as hc_compute_radiation; rad_Dlocal [D_local].  Needs hc_finalize.  HC_ERR_INVALID on a non-finite time or
 * velocity, on a second begin, on an end without a begin; nothing stays pending after a failed begin.  No owned body carries a
 * mode: zeros, and the ring is not touched. */
int hc_radiation_modes_begin(hc_ctx* ctx, double t, const double* linvel, const double* angvel);
int hc_radiation_modes_end(hc_ctx* ctx, double* rad_Dlocal);
int hc_compute_radiation_modes(hc_ctx* ctx, double t, const double* linvel, const double* angvel, double* rad_Dlocal);
/* Empties the ring (hc_reset_history calls it as well): the next call is a first call.  HC_ERR_INVALID while a begin is pending. */
int hc_reset_radiation_modes(hc_ctx* ctx);
/* sum Re[rho exp(lambda tau)] of the body's modes WITHOUT the rho factor, on the host: K [6][D][n_tau], what a fit is checked
 * against.  Any body of the system. */
int hc_get_radiation_modes_irf(hc_ctx* ctx, int body, int n_tau, const double* tau, double* K_6xDxn);

/* ------------------------------------------------------------------------------------------------
 * Synthetic many-body inputs generated directly in HBM (benchmark configurations C3/C4 of SURVEY 8d;
 * not part of the reference).  Fills K, K_hs, A_inf, excitation IRF for all local bodies from a
 * counter-based generator so that a 77 GB kernel never exists on the host.  hc_finalize still applies.
 * ---------------------------------------------------------------------------------------------- */
int hc_synth_fill(hc_ctx* ctx, unsigned long long seed, int S, double dt_rirf, int n_exc, double dt_exc);

#ifdef __cplusplus
}
#endif
#endif /* HYDROCHRONO_AMD_H */
