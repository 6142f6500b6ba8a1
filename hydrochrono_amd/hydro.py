"""HydroForces -- Python mirror of the reference's `TestHydro` surface (include/hydroc/hydro_forces.h:164-285),
implemented purely by calls into the C ABI (include/hydrochrono_amd.h).  No arithmetic happens here."""
import ctypes as C
from typing import Callable, NamedTuple

import numpy as np

from . import capi


class HydroError(RuntimeError):
    """A non-zero hc_status; .status holds it (1 = the reference throws std::runtime_error, 2 = std::out_of_range)."""

    def __init__(self, status, message):
        super().__init__(f"[hc_status={status}] {message}")
        self.status = status


def _dp(a):
    return None if a is None else a.ctypes.data_as(capi.c_double_p)


def _arr(x, n=None):
    a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} values, got {a.size}")
    return a


class HydroForces:
    def __init__(self, num_bodies, device=0, body_range=None):
        self.lib = capi.load()
        self.N = int(num_bodies)
        self.D = 6 * self.N
        self.b0, self.b1 = (0, self.N) if body_range is None else (int(body_range[0]), int(body_range[1]))
        self.n_local = self.b1 - self.b0
        self.D_local = 6 * self.n_local
        ctx = C.c_void_p()
        rc = self.lib.hc_create_sharded(self.N, self.b0, self.b1, int(device), C.byref(ctx))
        if rc != capi.HC_OK:
            raise HydroError(rc, self.lib.hc_last_error(None).decode())
        self.ctx = ctx

    # -- plumbing --
    def close(self):
        if getattr(self, "ctx", None):
            self.lib.hc_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != capi.HC_OK:
            raise HydroError(rc, self.lib.hc_last_error(self.ctx).decode())

    # -- ingest (H5FileInfo::ReadH5Data) --
    def load_bemio_h5(self, path):
        self._chk(self.lib.hc_load_bemio_h5(self.ctx, str(path).encode()))

    def set_simulation_parameters(self, rho, g, water_depth):
        self._chk(self.lib.hc_set_simulation_parameters(self.ctx, rho, g, water_depth))

    def set_body(self, b, disp_vol, cg, cb, lin, added_mass_inf, rirf_t, rirf_K):
        cg, cb, lin = _arr(cg, 3), _arr(cb, 3), _arr(lin, 36)
        A = _arr(added_mass_inf, 6 * self.D)
        t = _arr(rirf_t)
        K = _arr(rirf_K, 6 * self.D * t.size)
        self._chk(self.lib.hc_set_body_properties(self.ctx, b, float(disp_vol), _dp(cg), _dp(cb)))
        self._chk(self.lib.hc_set_hydrostatic_stiffness(self.ctx, b, _dp(lin)))
        self._chk(self.lib.hc_set_added_mass_inf(self.ctx, b, _dp(A)))
        self._chk(self.lib.hc_set_rirf(self.ctx, b, _dp(t), t.size, _dp(K)))

    def set_body_excitation_rao(self, b, w, mag, phase):
        w = _arr(w)
        mag, phase = _arr(mag, 6 * w.size), _arr(phase, 6 * w.size)
        self._chk(self.lib.hc_set_excitation_rao(self.ctx, b, _dp(w), w.size, _dp(mag), _dp(phase)))

    def set_body_excitation_irf(self, b, t, f):
        t = _arr(t)
        f = _arr(f, 6 * t.size)
        self._chk(self.lib.hc_set_excitation_irf(self.ctx, b, _dp(t), t.size, _dp(f)))

    def synth_fill(self, seed, S, dt_rirf, n_exc=0, dt_exc=0.0):
        self._chk(self.lib.hc_synth_fill(self.ctx, seed, S, dt_rirf, n_exc, dt_exc))

    def finalize(self):
        self._chk(self.lib.hc_finalize(self.ctx))

    @classmethod
    def from_case(cls, case, device=0, body_range=None):
        """Build from a raw-array case dict (see tests/cases.py, hydrochrono_amd/synthetic.py)."""
        h = cls(case["N"], device=device, body_range=body_range)
        h.set_simulation_parameters(case["rho"], case["g"], case["water_depth"])
        for b, bd in enumerate(case["bodies"]):
            h.set_body(b, bd["disp_vol"], bd["cg"], bd["cb"], bd["lin"], bd["added_mass_inf"], bd["rirf_t"], bd["rirf_K"])
            if "w" in bd:
                h.set_body_excitation_rao(b, bd["w"], bd["ex_mag"], bd["ex_phase"])
            if "ex_irf_t" in bd:
                h.set_body_excitation_irf(b, bd["ex_irf_t"], bd["ex_irf_f"])
        h.finalize()
        if "g_sys" in case:
            h.set_gravity(case["g_sys"])
        return h

    @classmethod
    def from_hydro_yaml(cls, yaml_path, system_body_names, timestep, sim_duration, ramp_duration=0.0, device=0):
        """ReadHydroYAML + SetupHydroFromYAML (src/hydro_yaml_parser.cpp, src/setup_hydro_from_yaml.cpp:126-193).
        Returns (HydroForces, matched_index) where matched_index[k] is the position of hydro body k in system_body_names."""
        lib = capi.load()
        cfg = C.c_void_p()
        err = C.create_string_buffer(2048)
        rc = lib.hc_yaml_read(str(yaml_path).encode(), C.byref(cfg), err, 2048)
        if rc != capi.HC_OK:
            raise HydroError(rc, err.value.decode())
        try:
            names = (C.c_char_p * len(system_body_names))(*[n.encode() for n in system_body_names])
            matched = (C.c_int * max(1, len(system_body_names)))()
            nm = C.c_int()
            ctx = C.c_void_p()
            rc = lib.hc_create_from_hydro_yaml(cfg, names, len(system_body_names), timestep, sim_duration, ramp_duration, int(device),
                                               C.byref(ctx), matched, C.byref(nm), err, 2048)
            if rc != capi.HC_OK:
                raise HydroError(rc, err.value.decode())
        finally:
            lib.hc_yaml_free(cfg)
        self = cls.__new__(cls)
        self.lib, self.ctx = lib, ctx
        self.N = nm.value
        self.D = 6 * self.N
        self.b0, self.b1, self.n_local, self.D_local = 0, self.N, self.N, self.D
        return self, list(matched[: nm.value])

    # -- configuration --
    def set_gravity(self, g3):
        g3 = _arr(g3, 3)
        self._chk(self.lib.hc_set_gravity(self.ctx, _dp(g3)))

    def add_waves_none(self, num_bodies=None):
        self._chk(self.lib.hc_set_wave_none(self.ctx, self.N if num_bodies is None else int(num_bodies)))

    def add_waves_regular(self, amplitude, omega, num_bodies=None):
        self._chk(self.lib.hc_set_wave_regular(self.ctx, self.N if num_bodies is None else int(num_bodies), amplitude, omega))

    def add_waves_irregular(self, simulation_dt, simulation_duration, ramp_duration=0.0, wave_height=0.0, wave_period=0.0,
                            frequency_min=0.001, frequency_max=1.0, nfrequencies=0, peak_enhancement_factor=1.0,
                            is_normalized=False, seed=1, num_bodies=None, spectral=False):
        p = capi.IrregularWaveParams()
        self.lib.hc_irregular_wave_params_default(C.byref(p))
        p.num_bodies = self.N if num_bodies is None else int(num_bodies)
        p.simulation_dt, p.simulation_duration, p.ramp_duration = simulation_dt, simulation_duration, ramp_duration
        p.wave_height, p.wave_period = wave_height, wave_period
        p.frequency_min, p.frequency_max, p.nfrequencies = frequency_min, frequency_max, nfrequencies
        p.peak_enhancement_factor, p.is_normalized, p.seed = peak_enhancement_factor, int(is_normalized), int(seed)
        fn = self.lib.hc_set_wave_irregular_spectral if spectral else self.lib.hc_set_wave_irregular
        self._chk(fn(self.ctx, C.byref(p)))

    def add_waves_irregular_eta(self, t, eta, simulation_dt, num_bodies=None):
        """IrregularWaves with eta_file_path_: the excitation convolution against an imported free-surface record (t strictly
        increasing, n >= 2), zero-extended over the excitation IRF; the IRF is resampled on simulation_dt.  See
        hc_set_wave_irregular_eta in include/hydrochrono_amd.h."""
        t = _arr(t)
        eta = _arr(eta, t.size)
        p = capi.IrregularWaveParams()
        self.lib.hc_irregular_wave_params_default(C.byref(p))
        p.num_bodies = self.N if num_bodies is None else int(num_bodies)
        p.simulation_dt = simulation_dt
        self._chk(self.lib.hc_set_wave_irregular_eta(self.ctx, C.byref(p), _dp(t), _dp(eta), t.size))

    def set_eta_record_components(self, f_min, f_max, max_components=0):
        """Give the imported record wave components: its discrete Fourier coefficients on its own grid inside [f_min, f_max] Hz,
        the max_components largest (0: all).  The wave kinematics and every side term then see that sea -- the periodic continuation
        of the record; the excitation convolution is not touched.  See hc_set_eta_record_components in include/hydrochrono_amd.h."""
        self._chk(self.lib.hc_set_eta_record_components(self.ctx, float(f_min), float(f_max), int(max_components)))

    def clear_eta_record_components(self):
        self._chk(self.lib.hc_clear_eta_record_components(self.ctx))

    def eta_record_components(self):
        """dict: m (bins), f [Hz], A, phase, k per kept component; mean, variance_share, rms_residual of the analysed samples."""
        n = C.c_int()
        s = [C.c_double() for _ in range(3)]
        self._chk(self.lib.hc_get_eta_record_components(self.ctx, C.byref(n), None, None, None, None, None, *[C.byref(x) for x in s]))
        m = np.zeros(n.value, dtype=np.int32)
        v = [np.zeros(n.value) for _ in range(4)]
        self._chk(self.lib.hc_get_eta_record_components(self.ctx, None, m.ctypes.data_as(capi.c_int_p), *[_dp(x) for x in v], None, None, None))
        return dict(m=m, f=v[0], A=v[1], phase=v[2], k=v[3], mean=s[0].value, variance_share=s[1].value, rms_residual=s[2].value)

    def set_eta_synthesis(self, mode):
        """0 = direct FP64 sum (default), 1 = rocFFT chirp-z."""
        self._chk(self.lib.hc_set_eta_synthesis(self.ctx, int(mode)))

    def set_convolution_mode(self, mode):
        self._chk(self.lib.hc_set_convolution_mode(self.ctx, int(mode)))

    def set_tapered_direct_options(self, smoothing=0, window_length=5, rirf_end_time=-1.0, taper_start_percent=0.8,
                                   taper_end_percent=1.0, taper_final_amplitude=0.0, export_plot_csv=False):
        o = capi.TaperedDirectOptions(int(smoothing), int(window_length), rirf_end_time, taper_start_percent,
                                      taper_end_percent, taper_final_amplitude, int(export_plot_csv))
        self._chk(self.lib.hc_set_tapered_direct_options(self.ctx, C.byref(o)))

    def set_diagnostics_output_directory(self, directory):
        self._chk(self.lib.hc_set_diagnostics_output_directory(self.ctx, str(directory).encode()))

    # -- per step --
    def step(self, t, pos, rpy, linvel, angvel):
        n3 = 3 * self.N
        a = [x if (type(x) is np.ndarray and x.dtype == np.float64 and x.size == n3 and x.flags.c_contiguous) else _arr(x, n3)
             for x in (pos, rpy, linvel, angvel)]
        out = np.empty(self.D_local)
        morison, nonlinear, drift = self.__dict__.get("_morison_any"), self._nonlinear_on(), self._drift_on()
        sumf = self._sum_on()
        radm = self.__dict__.get("_radm_any")
        if morison or nonlinear or drift or sumf or radm:
            # the side terms run on streams of their own beside the step; the composition is made here (the C ABI total stays the
            # reference's): the one-shard case of the driver that HydroGroup.step uses
            def step():
                return capi.step_raw(self.lib)(self.ctx, t, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, out.ctypes.data)
            return _step_with_side_terms(self, self, [(self.ctx, 0, self.D_local)], (nonlinear, morison, drift, sumf, radm), step, t, a, out,
                                         self.b0, self.b1)
        # raw addresses through a c_void_p prototype: this call sits in per-step loops
        rc = capi.step_raw(self.lib)(self.ctx, t, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, out.ctypes.data)
        if rc:
            self._chk(rc)
        return out

    def step_many(self, times, states, forces=None, seconds=None):
        """hc_step_many: one synchronous hc_step per row -- times [n], states [n][12N] packed pos | rpy | linvel | angvel
        (mock_chrono.PrescribedMotion.packed), both float64 C-contiguous -- in ONE call of the C ABI (a prescribed-motion driver's loop
        without an interpreter between the steps).  Returns (forces [n][D_local], seconds per call [n]); a failing step raises after
        the rows before it have been filled."""
        times = np.ascontiguousarray(times, dtype=np.float64)
        states = np.ascontiguousarray(states, dtype=np.float64)
        n = times.size
        if states.shape != (n, 12 * self.N):
            raise ValueError(f"states must be [{n}][{12 * self.N}]")
        forces = np.empty((n, self.D_local)) if forces is None else forces
        seconds = np.empty(n) if seconds is None else seconds
        # the C side writes n * D_local and n doubles through these pointers: anything but a writeable C-contiguous float64 array of
        # exactly that shape would be a heap overflow (or a silently ignored result), so refuse it -- also under python -O
        for name, arr, shape in (("forces", forces, (n, self.D_local)), ("seconds", seconds, (n,))):
            if not isinstance(arr, np.ndarray) or arr.dtype != np.float64 or arr.shape != shape or not arr.flags.c_contiguous or not arr.flags.writeable:
                raise ValueError(f"{name} must be a writeable C-contiguous float64 array of shape {shape}")
        done = C.c_int(0)
        rc = self.lib.hc_step_many(self.ctx, n, _dp(times), _dp(states), _dp(forces), _dp(seconds), C.byref(done))
        if rc:
            self._chk(rc)
        return forces, seconds

    def set_result_buffer(self, addr, size):
        """hc_set_result_buffer: the tagged {value, sequence} granules of hc_step go to caller memory at `addr` (e.g. a shared-memory
        segment other processes map, host_exchange.HostExchange); None / 0 hands the buffer back to the library."""
        self._chk(self.lib.hc_set_result_buffer(self.ctx, addr or None, int(size)))

    def step_sequence(self):
        """hc_step_sequence: the sequence number of the step begun last (what its granules are tagged with)."""
        s = C.c_ulonglong()
        self.lib.hc_step_sequence(self.ctx, C.byref(s))
        return s.value

    def step_device(self, t, state_ptr, out_ptr, stream_ptr=None):
        """state_ptr / out_ptr: integer device addresses (e.g. torch.Tensor.data_ptr()).

        stream_ptr: hipStream_t as an integer.  None or 0 is NOT the legacy default stream (whose handle is 0, e.g.
        torch.cuda.current_stream() outside a stream context) but the context's own non-blocking stream, which other
        work is not ordered against: pass an explicit stream (torch.cuda.Stream().cuda_stream) when device work of
        the caller -- a collective, a copy -- has to follow the step."""
        # plain ints go straight through the declared c_void_p argtypes (this call sits in per-step loops)
        rc = self.lib.hc_step_device(self.ctx, t, state_ptr, out_ptr, stream_ptr or None)
        if rc:
            self._chk(rc)

    def components(self):
        hs, rad, wv = (np.empty(self.D_local) for _ in range(3))
        self._chk(self.lib.hc_get_force_components(self.ctx, _dp(hs), _dp(rad), _dp(wv)))
        return hs, rad, wv

    def compute_radiation(self, t, linvel, angvel):
        lv, av = _arr(linvel, 3 * self.N), _arr(angvel, 3 * self.N)
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_compute_radiation(self.ctx, float(t), _dp(lv), _dp(av), _dp(out)))
        return out

    def compute_hydrostatics(self, pos, rpy):
        p, r = _arr(pos, 3 * self.N), _arr(rpy, 3 * self.N)
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_compute_hydrostatics(self.ctx, _dp(p), _dp(r), _dp(out)))
        return out

    def compute_waves(self, t):
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_compute_waves(self.ctx, float(t), _dp(out)))
        return out

    def set_lookahead(self, steps):
        """0 = plain per-step evaluation; > 0 = 16-step look-ahead blocking (the default)."""
        self._chk(self.lib.hc_set_lookahead(self.ctx, int(steps)))

    def set_pass_schedule(self, one_block_ahead, slices=0):
        """hc_set_pass_schedule: 0 = the pass of a look-ahead block when the block starts, 1 = one block ahead, in `slices` launches
        (0: chosen by the library) behind the first steps of the block before -- for callers that leave the GPU idle between force
        evaluations for less than a pass takes; None or -1 = the library's default: ADAPTIVE -- per block, from the gaps the caller
        left between the synchronous steps of the block before (back to back: at block start; away for more than a few
        microseconds: one block ahead; systems below 256 MB of K always at block start; HC_PASS_AHEAD=0/1 pins it)."""
        mode = -1 if one_block_ahead is None or int(one_block_ahead) < 0 else int(bool(one_block_ahead))
        self._chk(self.lib.hc_set_pass_schedule(self.ctx, mode, int(slices)))

    def set_radiation_tail(self, mode):
        """hc_set_radiation_tail: 1 (default) = lags from 128 on by partitioned FFT convolution in levels of doubling partition length
        where eligible (step = IRF spacing, full history, pass at block start, 6N < 1024, S >= 512); 2 = the uniform form (lags from
        256 on, partitions of 256); 0 = the full pass always."""
        self._chk(self.lib.hc_set_radiation_tail(self.ctx, int(mode)))

    def schedule(self):
        """hc_get_schedule: {"lookahead": 0 | 16 | 32 (what hc_set_lookahead made of its argument), "pass_schedule": -1 adaptive | 0 | 1,
        "ahead_now": the adaptive rule's current answer, "slices"}."""
        v = [C.c_int() for _ in range(4)]
        self._chk(self.lib.hc_get_schedule(self.ctx, *[C.byref(x) for x in v]))
        return dict(zip(("lookahead", "pass_schedule", "ahead_now", "slices"), (x.value for x in v)))

    def rirf_value(self, row_local, col, st):
        """TestHydro::GetRIRFval(row, col, st) for a local row (src/hydro_forces.cpp:693-711)."""
        v = C.c_double()
        self._chk(self.lib.hc_get_rirf_value(self.ctx, int(row_local), int(col), int(st), C.byref(v)))
        return v.value

    def direct_dispatch(self):
        """(active, reason): whether hc_step writes AQL packets itself instead of calling hipLaunchKernelGGL."""
        return bool(self.lib.hc_direct_dispatch_active(self.ctx)), self.lib.hc_dispatch_mode_reason(self.ctx).decode()

    def reset_history(self):
        self._chk(self.lib.hc_reset_history(self.ctx))

    def set_history(self, times_newest_first, vel):
        t = _arr(times_newest_first)
        v = _arr(vel, t.size * self.D)
        self._chk(self.lib.hc_set_history(self.ctx, t.size, _dp(t), _dp(v)))

    def get_history(self):
        n = C.c_int()
        self._chk(self.lib.hc_get_history(self.ctx, C.byref(n), None, None))
        t, v = np.empty(n.value), np.empty((n.value, self.D))
        self._chk(self.lib.hc_get_history(self.ctx, C.byref(n), _dp(t), _dp(v.reshape(-1))))
        return t, v

    # -- added mass (ChLoadAddedMass) --
    def added_mass_matrix(self):
        M = np.empty((self.D_local, self.D))
        self._chk(self.lib.hc_added_mass_matrix(self.ctx, _dp(M.reshape(-1))))
        return M

    def added_mass_mv(self, R, w, c):
        R = _arr(R).copy()
        w = _arr(w)
        self._chk(self.lib.hc_added_mass_mv(self.ctx, _dp(w), float(c), _dp(R), R.size))
        return R

    # -- introspection --
    def sizes(self):
        v = [C.c_int() for _ in range(8)]
        self._chk(self.lib.hc_get_sizes(self.ctx, *[C.byref(x) for x in v]))
        return dict(zip(("N", "n_local", "S", "L", "nf", "nt", "H", "Hcap"), (x.value for x in v)))

    def enable_profiling(self, on=1):
        """on = n > 0: HIP events around the kernels of every n-th step; 0/False: off."""
        self._chk(self.lib.hc_enable_profiling(self.ctx, int(on)))

    def reset_profile(self):
        self._chk(self.lib.hc_reset_profile(self.ctx))

    def profile(self):
        p = capi.ProfileStats()
        self._chk(self.lib.hc_get_profile(self.ctx, C.byref(p)))
        return {k: getattr(p, k) for k, _ in capi.ProfileStats._fields_}

    def init_stats(self):
        """hc_get_init_stats: what the init half of the path cost this context, stage by stage (seconds and bytes)."""
        st = capi.InitStats()
        self._chk(self.lib.hc_get_init_stats(self.ctx, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "pad_"}

    def rirf_width(self):
        w = np.empty(self.sizes()["S"])
        self._chk(self.lib.hc_get_rirf_width(self.ctx, _dp(w)))
        return w

    def rirf_effective(self):
        S = self.sizes()["S"]
        out = np.empty((self.D_local, self.D, S))
        self._chk(self.lib.hc_get_rirf_effective(self.ctx, _dp(out.reshape(-1))))
        return out

    def irreg_irf(self, b=0):
        Lb = C.c_int()
        self._chk(self.lib.hc_get_excitation_irf_size(self.ctx, b, C.byref(Lb)))
        L = Lb.value
        t, w, v = np.empty(L), np.empty(L), np.empty((6, L))
        self._chk(self.lib.hc_get_excitation_irf_resampled(self.ctx, b, _dp(t), _dp(w), _dp(v.reshape(-1))))
        return t, w, v

    def irreg_spectrum(self):
        nf = self.sizes()["nf"]
        arrs = [np.empty(nf) for _ in range(5)]
        self._chk(self.lib.hc_get_spectrum(self.ctx, *[_dp(a) for a in arrs]))
        return dict(zip(("f", "S", "df", "phase", "k"), arrs))

    def irreg_eta(self):
        nt = self.sizes()["nt"]
        t, e = np.empty(nt), np.empty(nt)
        self._chk(self.lib.hc_get_eta_table(self.ctx, _dp(t), _dp(e)))
        return t, e

    def export_irregular_inputs_h5(self, path):
        self._chk(self.lib.hc_export_irregular_inputs_h5(self.ctx, str(path).encode()))

    def regular_coeffs(self):
        mag, ph, k = np.empty(self.D), np.empty(self.D), C.c_double()
        self._chk(self.lib.hc_get_regular_coeffs(self.ctx, _dp(mag), _dp(ph), C.byref(k)))
        return mag, ph, k.value

    def simulation_parameters(self):
        rho, g, depth = C.c_double(), C.c_double(), C.c_double()
        self._chk(self.lib.hc_get_simulation_parameters(self.ctx, C.byref(rho), C.byref(g), C.byref(depth)))
        return rho.value, g.value, depth.value

    # -- wave kinematics (WaveBase::GetElevation / GetVelocity / GetAcceleration) --
    def wave_kinematics(self, points, times, mwl=0.0, regular_phase=0.0, wave_stretching=True):
        """Free-surface elevation, water velocity and acceleration of the wave model in force at every point (P x 3) and time (T):
        returns eta (T, P), vel (T, P, 3), acc (T, P, 3)."""
        xyz = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        t = _arr(times)
        P, T = xyz.shape[0], t.size
        eta, vel, acc = np.empty((T, P)), np.empty((T, P, 3)), np.empty((T, P, 3))
        o = capi.WaveKinematicsOpts()
        self.lib.hc_wave_kinematics_opts_default(C.byref(o))
        o.mwl, o.regular_phase, o.wave_stretching = float(mwl), float(regular_phase), int(bool(wave_stretching))
        self._chk(self.lib.hc_wave_kinematics(self.ctx, C.byref(o), P, _dp(xyz.reshape(-1)), T, _dp(t), _dp(eta.reshape(-1)),
                                              _dp(vel.reshape(-1)), _dp(acc.reshape(-1))))
        return eta, vel, acc

    # -- wave heading and short-crested seas (an extension beyond the reference, which ignores waves.direction) --
    def set_wave_directions(self, theta=None):
        """One direction [rad, 0 along +x, positive towards +y] per component of the wave model in force (1 for a regular wave, else
        nf); None or empty clears them.  Every add_waves_* call drops them.  See hc_set_wave_directions in include/hydrochrono_amd.h."""
        th = np.zeros(0) if theta is None else _arr(theta)
        self._chk(self.lib.hc_set_wave_directions(self.ctx, th.size, _dp(th) if th.size else None))

    def wave_directions(self):
        """The directions in force, (n,); empty when none are set."""
        n = C.c_int()
        self._chk(self.lib.hc_get_wave_directions(self.ctx, C.byref(n), None))
        th = np.empty(n.value)
        if n.value:
            self._chk(self.lib.hc_get_wave_directions(self.ctx, C.byref(n), _dp(th)))
        return th

    def set_wave_spreading(self, heading, s=0.0, n_bins=15, seed=1):
        """Equal-energy directions of the cos-2s spreading about `heading` for the wave model in force (s <= 0: the uniform heading),
        then set_wave_directions.  Returns the directions."""
        th = wave_spreading_directions(self.wave_component_count(), heading, s, n_bins, seed, lib=self.lib)
        self.set_wave_directions(th)
        return th

    def set_body_excitation_rao_headings(self, b, dirs, w, mag, phase):
        """Excitation coefficients of body b on a grid of headings: dirs (n_dir,) strictly increasing [rad], w (nw,), mag and phase
        (6, n_dir, nw), the layout of a BEMIO file; empty dirs remove them."""
        dirs, w = _arr(dirs), _arr(w)
        mag, phase = _arr(mag, 6 * dirs.size * w.size), _arr(phase, 6 * dirs.size * w.size)
        self._chk(self.lib.hc_set_excitation_rao_headings(self.ctx, b, dirs.size, _dp(dirs), _dp(w), w.size, _dp(mag), _dp(phase)))

    def excitation_rao_headings_size(self, b):
        nd, nw = C.c_int(), C.c_int()
        self._chk(self.lib.hc_get_excitation_rao_headings_size(self.ctx, b, C.byref(nd), C.byref(nw)))
        return nd.value, nw.value

    # -- second-order irregular waves (Sharma and Dean; an extension beyond the reference) --
    def _wave2_opts(self, mwl, regular_phase, diff_band, sum_band, apply_ramp):
        o = capi.WaveKinematics2Opts()
        self.lib.hc_wave_kinematics2_opts_default(C.byref(o))
        o.mwl, o.regular_phase, o.apply_ramp = float(mwl), float(regular_phase), int(bool(apply_ramp))
        (o.diff_lo, o.diff_hi), (o.sum_lo, o.sum_hi) = map(float, diff_band), map(float, sum_band)
        return o

    def wave_kinematics2(self, points, times, mwl=0.0, regular_phase=0.0, diff_band=(0.0, float("inf")), sum_band=(0.0, float("inf")),
                         apply_ramp=True, directional=False):
        """The second-order increments to wave_kinematics() at every point (P x 3) and time (T): eta2 (T, P), vel2 (T, P, 3),
        acc2 (T, P, 3); the caller adds them to the first-order values.  diff_band / sum_band: (lo, hi) in rad/s of the
        difference and sum frequencies that take part.  See hc_wave_kinematics2 in include/hydrochrono_amd.h.
        directional=True: the short-crested sea of set_wave_directions() (hc_wave_kinematics2_dir); the default is the long-crested
        call, which refuses while directions are set."""
        xyz = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        t = _arr(times)
        P, T = xyz.shape[0], t.size
        eta, vel, acc = np.empty((T, P)), np.empty((T, P, 3)), np.empty((T, P, 3))
        o = self._wave2_opts(mwl, regular_phase, diff_band, sum_band, apply_ramp)
        call = self.lib.hc_wave_kinematics2_dir if directional else self.lib.hc_wave_kinematics2
        self._chk(call(self.ctx, C.byref(o), P, _dp(xyz.reshape(-1)), T, _dp(t), _dp(eta.reshape(-1)), _dp(vel.reshape(-1)), _dp(acc.reshape(-1))))
        return eta, vel, acc

    def wave_pair_tables(self, regular_phase=0.0, diff_band=(0.0, float("inf")), sum_band=(0.0, float("inf")), directional=False):
        """The device's pair tables of wave_kinematics2(): dict of Kp, Km, Bp, Bm, (nf, nf) each, zero outside the bands;
        directional=True: those of the short-crested sea (hc_wave_kinematics2_dir_pair_tables)."""
        nf = self.wave_component_count()
        out = {n: np.zeros((nf, nf)) for n in ("Kp", "Km", "Bp", "Bm")}
        o = self._wave2_opts(0.0, regular_phase, diff_band, sum_band, True)
        call = self.lib.hc_wave_kinematics2_dir_pair_tables if directional else self.lib.hc_wave_kinematics2_pair_tables
        self._chk(call(self.ctx, C.byref(o), *[_dp(out[n].reshape(-1)) for n in ("Kp", "Km", "Bp", "Bm")]))
        return out

    def wave_component_count(self):
        """Components of the wave model in force as the kinematics see them: nf of the spectrum, 1 for a regular wave, else 0."""
        if self.lib.hc_get_regular_coeffs(self.ctx, None, None, None) == capi.HC_OK:
            return 1
        return self.sizes()["nf"]

    # -- Morison drag and inertia elements (an extension beyond the reference) --
    def set_morison_elements(self, b, r, cd_area, cm_vol):
        """Replaces the element list of body b (0-based): r, cd_area, cm_vol are (n, 3) -- positions in the body frame, Cd_i A_i [m^2]
        and Cm_i V [m^3] per body axis; empty arrays clear it.  From then on step() returns total + Morison term."""
        r, cd, cm = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3) for x in (r, cd_area, cm_vol))
        if not (r.shape == cd.shape == cm.shape):
            raise ValueError("r, cd_area and cm_vol must have the same shape (n, 3)")
        n = r.shape[0]
        elems = (capi.MorisonElement * max(n, 1))()
        flat = np.concatenate([r, cd, cm], axis=1)
        if n:
            C.memmove(elems, flat.ctypes.data, flat.nbytes)
        self._chk(self.lib.hc_set_morison_elements(self.ctx, int(b), elems, n))
        counts = self.__dict__.setdefault("_morison_counts", {})
        counts[int(b)] = n
        self._morison_any = any(counts.values()) or any(self.__dict__.get("_morison_member_counts", {}).values())

    def set_morison_members(self, b, r0, r1, diameter, cd, cm, n_seg):
        """Replaces the strip-member list of body b (0-based): r0, r1 are (n, 3) end points in the body frame; diameter is a scalar,
        (n,) or (n, 2) (at r0 and at r1, linear in between); cd, cm, n_seg are scalars or (n,).  Empty arrays clear the list.  A
        body with members counts as one that carries elements: step() returns total + Morison term (elements + members)."""
        r0, r1 = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3) for x in (r0, r1))
        if r0.shape != r1.shape:
            raise ValueError("r0 and r1 must have the same shape (n, 3)")
        n = r0.shape[0]
        dia = np.asarray(diameter, dtype=np.float64)
        dia = np.broadcast_to(dia[:, None] if dia.ndim == 1 else dia, (n, 2))
        cd, cm = (np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)) for x in (cd, cm))
        seg = np.broadcast_to(np.asarray(n_seg), (n,))
        if np.any(seg != np.floor(seg)):
            raise ValueError("n_seg must be whole numbers")
        members = (capi.MorisonMember * max(n, 1))()
        for e in range(n):
            m = members[e]
            m.r0[:], m.r1[:] = r0[e], r1[e]
            m.d0, m.d1, m.cd, m.cm, m.n_seg = dia[e, 0], dia[e, 1], cd[e], cm[e], int(seg[e])
        self._chk(self.lib.hc_set_morison_members(self.ctx, int(b), members, n))
        counts = self.__dict__.setdefault("_morison_member_counts", {})
        counts[int(b)] = n
        self._morison_any = any(counts.values()) or any(self.__dict__.get("_morison_counts", {}).values())

    def morison_member_count(self, b):
        n = C.c_int()
        self._chk(self.lib.hc_get_morison_member_count(self.ctx, int(b), C.byref(n)))
        return n.value

    def morison_member_forces(self, b):
        """The 6-vectors (n, 6) of the members of body b (0-based, owned) in the last completed evaluation; their serial sum in
        member order is the body's member part, bit for bit."""
        out = np.empty((self.morison_member_count(b), 6))
        self._chk(self.lib.hc_get_morison_member_forces(self.ctx, int(b), _dp(out.reshape(-1)) if out.size else _dp(np.empty(1))))
        return out

    def set_morison_member_added_mass(self, b, ca):
        """The added-mass coefficients ca >= 0 of the members of body b (0-based): a scalar or (n,) with n the body's member count;
        None or an empty array clears them, and set_morison_members() resets them to 0.  From the next Morison evaluation on,
        morison_added_mass() returns the body's 6 x 6 added-mass matrix on the instantaneous wet length; the forces do not change.
        See hc_set_morison_member_added_mass in include/hydrochrono_amd.h."""
        n = self.morison_member_count(b)
        ca = np.zeros(0) if ca is None else np.ascontiguousarray(np.broadcast_to(np.asarray(ca, dtype=np.float64), (n,)) if np.ndim(ca) == 0
                                                                 else np.asarray(ca, dtype=np.float64).reshape(-1))
        self._chk(self.lib.hc_set_morison_member_added_mass(self.ctx, int(b), _dp(ca) if ca.size else None, int(ca.size)))

    def morison_member_added_mass_coefficients(self, b):
        ca = np.zeros(self.morison_member_count(b))
        self._chk(self.lib.hc_get_morison_member_added_mass_coefficients(self.ctx, int(b), _dp(ca) if ca.size else None))
        return ca

    def morison_added_mass(self, body=None):
        """The added-mass matrix (6, 6) of body `body` (0-based, owned) in the last completed Morison evaluation, in world axes at
        the body's reference point; body=None: (N_local, 6, 6) over the owned bodies.  A body no member of which has ca > 0 gives
        zeros."""
        if body is None:
            return np.stack([self.morison_added_mass(b) for b in range(self.b0, self.b1)])
        M = np.zeros((6, 6))
        if np.any(self.morison_member_added_mass_coefficients(body) > 0.0):
            self._chk(self.lib.hc_get_morison_added_mass(self.ctx, int(body), _dp(M.reshape(-1))))
        return M

    def morison_member_added_mass(self, b):
        """The matrices (n, 6, 6) of the members of body b (0-based, owned) in the last completed evaluation; their serial sum in
        member order is morison_added_mass(b), bit for bit.  Zeros as well for a body no member of which has ca > 0."""
        out = np.zeros((self.morison_member_count(b), 6, 6))
        if np.any(self.morison_member_added_mass_coefficients(b) > 0.0):
            self._chk(self.lib.hc_get_morison_member_added_mass(self.ctx, int(b), _dp(out.reshape(-1))))
        return out

    def morison_added_mass_force(self, linacc, angacc):
        """-M (a_lin, alpha) per owned body, (N_local, 6), on the host from morison_added_mass(): the body-acceleration term of
        Morison's equation for a caller without a mass-matrix hook (the centripetal part is left out).  linacc, angacc: the
        accelerations of all bodies of the system, (N, 3) in world axes."""
        n3 = 3 * self.N
        acc = np.concatenate([_arr(linacc, n3).reshape(-1, 3), _arr(angacc, n3).reshape(-1, 3)], axis=1)[self.b0:self.b1]
        return -np.matmul(self.morison_added_mass(), acc[:, :, None])[:, :, 0]

    def set_morison_members_second_order(self, on=True):
        """With set_morison_second_order() on, the strip members see the second-order sea as well: eta2 at every node moves the cut,
        u2 and a2 at the Gauss points the cut yields enter the drag product and the inertia term (in a directional sea, with
        set_morison_second_order_directional(), those of wave_kinematics2(directional=True)).  Off (the default), an evaluation
        with members on the second-order sea refuses.  A switch of its own, kept when the other two change.  See
        hc_set_morison_members_second_order in include/hydrochrono_amd.h."""
        self._chk(self.lib.hc_set_morison_members_second_order(self.ctx, int(bool(on))))

    def morison_members_second_order(self):
        on = C.c_int()
        self._chk(self.lib.hc_get_morison_members_second_order(self.ctx, C.byref(on)))
        return bool(on.value)

    def morison_member_increments(self, b):
        """What the members of body b (0-based, owned) saw in the last evaluation on the second-order sea, over its members in index
        order: dict of node_p (sum(n_seg + 1), 3), node_eta2, and of the Gauss points p (sum(2 n_seg), 3), eta2, vel2, acc2 (zeros
        behind the point of a dry segment; the y components are zero after a long-crested evaluation)."""
        nn, npt = C.c_int(), C.c_int()
        self._chk(self.lib.hc_get_morison_member_increment_counts(self.ctx, int(b), C.byref(nn), C.byref(npt)))
        nn, npt = nn.value, npt.value
        out = dict(node_p=np.empty((nn, 3)), node_eta2=np.empty(nn), p=np.empty((npt, 3)), eta2=np.empty(npt), vel2=np.empty((npt, 3)),
                   acc2=np.empty((npt, 3)))
        self._chk(self.lib.hc_get_morison_member_node_increments(self.ctx, int(b), *[_dp(out[k].reshape(-1)) for k in ("node_p", "node_eta2")]))
        self._chk(self.lib.hc_get_morison_member_point_increments(self.ctx, int(b), *[_dp(out[k].reshape(-1)) for k in ("p", "eta2", "vel2", "acc2")]))
        return out

    def morison_count(self, b):
        n = C.c_int()
        self._chk(self.lib.hc_get_morison_count(self.ctx, int(b), C.byref(n)))
        return n.value

    def set_morison_options(self, mwl=0.0, regular_phase=0.0, wave_stretching=True):
        """mwl, regular_phase, wave_stretching of the wave kinematics the elements see (those of wave_kinematics())."""
        o = capi.WaveKinematicsOpts(float(mwl), float(regular_phase), int(bool(wave_stretching)))
        self._chk(self.lib.hc_set_morison_options(self.ctx, C.byref(o)))

    def set_morison_second_order(self, on=True, diff_band=(0.0, float("inf")), sum_band=(0.0, float("inf")), apply_ramp=True):
        """The elements see the second-order increments of wave_kinematics2() on top of the first-order field (eta1 + eta2 in the
        wet test, u1 + u2 and a1 + a2 in the force); diff_band / sum_band: (lo, hi) in rad/s as there, mwl and regular_phase from
        set_morison_options().  on=False frees the tables.  See hc_set_morison_second_order in include/hydrochrono_amd.h."""
        (dlo, dhi), (slo, shi) = map(float, diff_band), map(float, sum_band)
        self._chk(self.lib.hc_set_morison_second_order(self.ctx, int(bool(on)), dlo, dhi, slo, shi, int(bool(apply_ramp))))

    def morison_second_order(self):
        """dict(on, diff_band, sum_band, apply_ramp) as set_morison_second_order() takes them."""
        on, ramp = C.c_int(), C.c_int()
        v = [C.c_double() for _ in range(4)]
        self._chk(self.lib.hc_get_morison_second_order(self.ctx, C.byref(on), *[C.byref(x) for x in v], C.byref(ramp)))
        return dict(on=bool(on.value), diff_band=(v[0].value, v[1].value), sum_band=(v[2].value, v[3].value), apply_ramp=bool(ramp.value))

    def set_morison_second_order_directional(self, on=True):
        """With set_morison_second_order() on and wave directions set, the elements see the increments of
        wave_kinematics2(directional=True) -- u2 and a2 with their y components -- where the evaluation otherwise refuses.  A switch
        of its own, kept when second order goes off and on; without directions it changes nothing.  See
        hc_set_morison_second_order_directional in include/hydrochrono_amd.h."""
        self._chk(self.lib.hc_set_morison_second_order_directional(self.ctx, int(bool(on))))

    def morison_second_order_directional(self):
        on = C.c_int()
        self._chk(self.lib.hc_get_morison_second_order_directional(self.ctx, C.byref(on)))
        return bool(on.value)

    def morison_increments(self, b):
        """What the elements of body b (0-based, owned) saw in the last evaluation on the second-order sea: dict of p (n, 3),
        eta2 (n), vel2 (n, 3), acc2 (n, 3); the y components are zero after a long-crested evaluation."""
        n = self.morison_count(b)
        out = dict(p=np.empty((n, 3)), eta2=np.empty(n), vel2=np.empty((n, 3)), acc2=np.empty((n, 3)))
        self._chk(self.lib.hc_get_morison_increments(self.ctx, int(b), *[_dp(out[k].reshape(-1)) for k in ("p", "eta2", "vel2", "acc2")]))
        return out

    def morison_begin(self, t, pos, rpy, linvel, angvel):
        n3 = 3 * self.N
        a = [_arr(x, n3) for x in (pos, rpy, linvel, angvel)]
        self._chk(self.lib.hc_morison_begin(self.ctx, float(t), _dp(a[0]), _dp(a[1]), _dp(a[2]), _dp(a[3])))

    def morison_end(self):
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_morison_end(self.ctx, _dp(out)))
        return out

    def compute_morison(self, t, pos, rpy, linvel, angvel):
        """The Morison 6-vectors of the owned bodies (world frame, at the body reference) for the given state; zeros without elements."""
        n3 = 3 * self.N
        a = [_arr(x, n3) for x in (pos, rpy, linvel, angvel)]
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_compute_morison(self.ctx, float(t), _dp(a[0]), _dp(a[1]), _dp(a[2]), _dp(a[3]), _dp(out)))
        return out

    def morison(self):
        """The Morison term of the last step() (zeros when no element is set)."""
        m = self.__dict__.get("_morison_last")
        return np.zeros(self.D_local) if m is None or not self.__dict__.get("_morison_any") else m.copy()

    # -- nonlinear buoyancy and Froude-Krylov forces on surface panels (an extension beyond the reference) --
    def set_surface_panels(self, b, c, s):
        """Replaces the panel list of body b (0-based): c, s are (n, 3) -- centroids [m] and area vectors [m^2] (area times the outward
        normal, body into water) in the body frame; empty arrays clear it.  With set_nonlinear_mode(1 or 2) step() then replaces the
        body's linear hydrostatic term by the pressure integral over the wetted panels."""
        c, s = (np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3) for x in (c, s))
        if c.shape != s.shape:
            raise ValueError("c and s must have the same shape (n, 3)")
        n = c.shape[0]
        panels = (capi.SurfacePanel * max(n, 1))()
        flat = np.concatenate([c, s], axis=1)
        if n:
            C.memmove(panels, flat.ctypes.data, flat.nbytes)
        self._chk(self.lib.hc_set_surface_panels(self.ctx, int(b), panels, n))
        self.__dict__.setdefault("_panel_counts", {})[int(b)] = n

    def set_surface_mesh(self, b, triangles, clip=False):
        """Panels from triangles [n][3][3] (vertices in the body frame, counter-clockwise seen from the water):
        c = (v0 + v1 + v2) / 3, s = 1/2 (v1 - v0) x (v2 - v0).  clip=True keeps the vertices instead (hc_set_surface_triangles): every
        triangle is cut at the instantaneous free surface, so the force is continuous in the state and exact in still water.  A body
        carries panels or triangles: either call replaces what the body carried."""
        if not clip:
            c, s = triangles_to_panels(triangles)
            self.set_surface_panels(b, c, s)
            return
        tri = np.ascontiguousarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
        n = tri.shape[0]
        self._chk(self.lib.hc_set_surface_triangles(self.ctx, int(b), _dp(tri if n else np.zeros(9)), n))
        self.__dict__.setdefault("_panel_counts", {})[int(b)] = n  # the body's one list, of either kind

    def surface_panel_count(self, b):
        n = C.c_int()
        self._chk(self.lib.hc_get_surface_panel_count(self.ctx, int(b), C.byref(n)))
        return n.value

    def surface_triangle_count(self, b):
        n = C.c_int()
        self._chk(self.lib.hc_get_surface_triangle_count(self.ctx, int(b), C.byref(n)))
        return n.value

    def set_nonlinear_options(self, mwl=0.0, regular_phase=0.0, wave_stretching=True):
        """mwl, regular_phase, wave_stretching of the wave kinematics the panels see (those of wave_kinematics())."""
        o = capi.WaveKinematicsOpts(float(mwl), float(regular_phase), int(bool(wave_stretching)))
        self._chk(self.lib.hc_set_nonlinear_options(self.ctx, C.byref(o)))

    def set_nonlinear_second_order(self, on=True, diff_band=(0.0, float("inf")), sum_band=(0.0, float("inf")), apply_ramp=True):
        """The panels and clipped triangles on the second-order sea: eta1 + eta2 in the wet test and the clipping height, and
        rho q2 - 1/2 rho ramp^2 |u1|^2 added to p_d (q2 = -d phi2 / dt); diff_band / sum_band: (lo, hi) in rad/s as wave_kinematics2()
        takes them, mwl and regular_phase from set_nonlinear_options().  on=False frees the tables.  See
        hc_set_nonlinear_second_order in include/hydrochrono_amd.h."""
        (dlo, dhi), (slo, shi) = map(float, diff_band), map(float, sum_band)
        self._chk(self.lib.hc_set_nonlinear_second_order(self.ctx, int(bool(on)), dlo, dhi, slo, shi, int(bool(apply_ramp))))

    def nonlinear_second_order(self):
        """dict(on, diff_band, sum_band, apply_ramp) as set_nonlinear_second_order() takes them."""
        on, ramp = C.c_int(), C.c_int()
        v = [C.c_double() for _ in range(4)]
        self._chk(self.lib.hc_get_nonlinear_second_order(self.ctx, C.byref(on), *[C.byref(x) for x in v], C.byref(ramp)))
        return dict(on=bool(on.value), diff_band=(v[0].value, v[1].value), sum_band=(v[2].value, v[3].value), apply_ramp=bool(ramp.value))

    def set_nonlinear_second_order_directional(self, on=True):
        """With set_nonlinear_second_order() on and wave directions set, the surface points see eta2 and q2 of
        wave_kinematics2(directional=True)'s pair sum and |u1|^2 with its y component, where the evaluation otherwise refuses.  A
        switch of its own, kept when second order goes off and on; without directions it changes nothing.  See
        hc_set_nonlinear_second_order_directional in include/hydrochrono_amd.h."""
        self._chk(self.lib.hc_set_nonlinear_second_order_directional(self.ctx, int(bool(on))))

    def nonlinear_second_order_directional(self):
        on = C.c_int()
        self._chk(self.lib.hc_get_nonlinear_second_order_directional(self.ctx, C.byref(on)))
        return bool(on.value)

    def nonlinear_point_count(self, b):
        """The distinct surface points of body b (0-based): panel centroids or triangle vertices, a shared vertex once."""
        n = C.c_int()
        self._chk(self.lib.hc_get_nonlinear_point_count(self.ctx, int(b), C.byref(n)))
        return n.value

    def nonlinear_increments(self, b):
        """What the surface points of body b (0-based, owned) saw in the last evaluation on the second-order sea: dict of p (n, 3),
        eta2 (n), q2 (n), one entry per distinct point in the order of its first use."""
        n = self.nonlinear_point_count(b)
        out = dict(p=np.empty((n, 3)), eta2=np.empty(n), q2=np.empty(n))
        self._chk(self.lib.hc_get_nonlinear_increments(self.ctx, int(b), n, *[_dp(out[k].reshape(-1)) for k in ("p", "eta2", "q2")]))
        return out

    def set_nonlinear_mode(self, mode):
        """0: off (step() as without panels); 1: a body with panels gets total - hs_lin + buoy; 2: total - hs_lin + buoy + fk (the
        excitation data of the context should then be the scattering part only: nothing is subtracted from the wave term)."""
        if int(mode) not in (0, 1, 2):
            raise ValueError("nonlinear mode must be 0, 1 or 2")
        self._nonlinear_mode = int(mode)

    def _nonlinear_on(self):
        d = self.__dict__  # _panel_counts: the size of every body's list, panels or triangles (a setter of one kind clears the other)
        return bool(d.get("_nonlinear_mode")) and any(d.get("_panel_counts", {}).values())

    def compute_nonlinear(self, t, pos, rpy):
        """(buoy, fk, hs_lin) of the owned bodies (D_local each; world frame, at the body reference) for the given state."""
        n3 = 3 * self.N
        a = [_arr(x, n3) for x in (pos, rpy)]
        out = tuple(np.empty(self.D_local) for _ in range(3))
        self._chk(self.lib.hc_compute_nonlinear(self.ctx, float(t), _dp(a[0]), _dp(a[1]), _dp(out[0]), _dp(out[1]), _dp(out[2])))
        return out

    def nonlinear_begin(self, t, pos, rpy):
        n3 = 3 * self.N
        a = [_arr(x, n3) for x in (pos, rpy)]
        self._chk(self.lib.hc_nonlinear_begin(self.ctx, float(t), _dp(a[0]), _dp(a[1])))

    def nonlinear_end(self):
        out = tuple(np.empty(self.D_local) for _ in range(3))
        self._chk(self.lib.hc_nonlinear_end(self.ctx, _dp(out[0]), _dp(out[1]), _dp(out[2])))
        return out

    def nonlinear(self):
        """(buoy, fk, hs_lin) of the last step() (zeros when the mode is 0 or no panel is set)."""
        m = self.__dict__.get("_nonlinear_last")
        if m is None or not self._nonlinear_on():
            return tuple(np.zeros(self.D_local) for _ in range(3))
        return tuple(x.copy() for x in m)

    # -- second-order wave drift forces from QTF tables (an extension beyond the reference) --
    def _set_qtf(self, setter, setter_headings, b, omega, P, Q, headings):
        omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
        nq = omega.size
        if nq == 0:
            self._chk(setter(self.ctx, int(b), 0, None, None, None))
            return 0
        P = np.ascontiguousarray(P, dtype=np.float64)
        Q = None if Q is None else np.ascontiguousarray(Q, dtype=np.float64)
        if headings is None:
            if P.size != 6 * nq * nq or (Q is not None and Q.size != 6 * nq * nq):
                raise ValueError("P and Q must have shape (6, nq, nq)")
            self._chk(setter(self.ctx, int(b), nq, _dp(omega), _dp(P), None if Q is None else _dp(Q)))
        else:
            beta = np.ascontiguousarray(headings, dtype=np.float64).reshape(-1)
            shape = (6, beta.size, beta.size, nq, nq)
            if P.shape != shape or (Q is not None and Q.shape != shape):
                raise ValueError("with headings, P and Q must have shape (6, nh, nh, nq, nq)")
            self._chk(setter_headings(self.ctx, int(b), beta.size, _dp(beta), nq, _dp(omega), _dp(P), None if Q is None else _dp(Q)))
        return nq

    def set_drift_qtf(self, b, omega, P, Q=None, headings=None):
        """Replaces the difference-frequency QTF table of body b (0-based): omega [nq] rad/s, strictly increasing, 2 <= nq <= 256;
        P, Q [6][nq][nq] real and imaginary part, force (moment) per squared amplitude, dimensional; Q=None means zeros; an empty
        omega clears the table.  With set_drift_mode(1, 2 or 3) step() then returns total + drift term.
        headings [nh] rad (world frame, strictly increasing, nh <= 16, nh nq <= 1024): a table on a heading grid, P, Q of shape
        (6, nh, nh, nq, nq), element (d, a, b, m, n) = T(beta_a, beta_b, Omega_m, Omega_n); the one kind of table that is evaluated
        while wave directions are set (hc_set_drift_qtf_headings)."""
        nq = self._set_qtf(self.lib.hc_set_drift_qtf, self.lib.hc_set_drift_qtf_headings, b, omega, P, Q, headings)
        self.__dict__.setdefault("_drift_sizes", {})[int(b)] = nq

    def set_drift_mean(self, b, omega, D, headings=None):
        """Mean-drift coefficients D [6][nq] on omega [nq]: a table with D on the diagonal and zeros elsewhere, for modes 1 and 2
        (mode 3 needs a full table: it would take the zeros off the diagonal as data).  With headings [nh]: D of shape (6, nh, nq)."""
        omega = np.ascontiguousarray(omega, dtype=np.float64).reshape(-1)
        nq = omega.size
        D = np.ascontiguousarray(D, dtype=np.float64)
        if headings is None:
            if D.shape != (6, nq):
                raise ValueError("D must have shape (6, nq)")
            P = np.zeros((6, nq, nq))
            P[:, np.arange(nq), np.arange(nq)] = D
        else:
            nh = np.size(headings)
            if D.shape != (6, nh, nq):
                raise ValueError("with headings, D must have shape (6, nh, nq)")
            P = np.zeros((6, nh, nh, nq, nq))
            for a in range(nh):
                P[:, a, a, np.arange(nq), np.arange(nq)] = D[:, a]
        self.set_drift_qtf(b, omega, P, headings=headings)

    def drift_qtf_size(self, b):
        n = C.c_int()
        self._chk(self.lib.hc_get_drift_qtf_size(self.ctx, int(b), C.byref(n)))
        return n.value

    def drift_qtf_headings(self, b):
        """The heading count of body b's drift table: 0 for a one-heading table or none."""
        n = C.c_int()
        self._chk(self.lib.hc_get_drift_qtf_headings(self.ctx, int(b), C.byref(n)))
        return n.value

    def set_drift_mode(self, mode):
        """0: off; 1: mean drift; 2: Newman's approximation; 3: full QTF."""
        self._chk(self.lib.hc_set_drift_mode(self.ctx, int(mode)))
        self._drift_mode = int(mode)

    def set_drift_options(self, regular_phase=0.0):
        """The phase of a regular wave as the drift term sees it (that of wave_kinematics())."""
        o = capi.WaveKinematicsOpts(0.0, float(regular_phase), 1)
        self._chk(self.lib.hc_set_drift_options(self.ctx, C.byref(o)))

    def _drift_on(self):
        d = self.__dict__
        return bool(d.get("_drift_mode")) and any(d.get("_drift_sizes", {}).values())

    def compute_drift(self, t, pos):
        """The drift 6-vectors of the owned bodies (world frame, at the body reference) at time t and positions pos; zeros with
        mode 0, without a table, and without wave components."""
        a = _arr(pos, 3 * self.N)
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_compute_drift(self.ctx, float(t), _dp(a), _dp(out)))
        return out

    def drift_begin(self, t, pos):
        a = _arr(pos, 3 * self.N)
        self._chk(self.lib.hc_drift_begin(self.ctx, float(t), _dp(a)))

    def drift_end(self):
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_drift_end(self.ctx, _dp(out)))
        return out

    def drift(self):
        """The drift term of the last step() (zeros when the mode is 0 or no table is set)."""
        m = self.__dict__.get("_drift_last")
        return np.zeros(self.D_local) if m is None or not self._drift_on() else m.copy()

    # -- second-order wave forces from sum-frequency QTF tables (an extension beyond the reference) --
    def set_sum_qtf(self, b, omega, P, Q=None, headings=None):
        """Replaces the sum-frequency QTF table of body b (0-based): omega [nq] rad/s, a grid of its own, strictly increasing,
        2 <= nq <= 256; P, Q [6][nq][nq] real and imaginary part, force (moment) per squared amplitude, dimensional; Q=None means
        zeros; an empty omega clears the table.  Only the symmetric part of a table can contribute.  With set_sum_mode(1) step() then
        returns total (+ drift term) + sum-frequency term.  headings: as set_drift_qtf (hc_set_sum_qtf_headings)."""
        nq = self._set_qtf(self.lib.hc_set_sum_qtf, self.lib.hc_set_sum_qtf_headings, b, omega, P, Q, headings)
        self.__dict__.setdefault("_sum_sizes", {})[int(b)] = nq

    def sum_qtf_size(self, b):
        n = C.c_int()
        self._chk(self.lib.hc_get_sum_qtf_size(self.ctx, int(b), C.byref(n)))
        return n.value

    def sum_qtf_headings(self, b):
        """The heading count of body b's sum-frequency table: 0 for a one-heading table or none."""
        n = C.c_int()
        self._chk(self.lib.hc_get_sum_qtf_headings(self.ctx, int(b), C.byref(n)))
        return n.value

    def set_sum_mode(self, mode):
        """0: off; 1: on."""
        self._chk(self.lib.hc_set_sum_mode(self.ctx, int(mode)))
        self._sum_mode = int(mode)

    def set_sum_options(self, regular_phase=0.0):
        """The phase of a regular wave as the sum-frequency term sees it (that of wave_kinematics())."""
        o = capi.WaveKinematicsOpts(0.0, float(regular_phase), 1)
        self._chk(self.lib.hc_set_sum_options(self.ctx, C.byref(o)))

    def _sum_on(self):
        d = self.__dict__
        return bool(d.get("_sum_mode")) and any(d.get("_sum_sizes", {}).values())

    def compute_sum_qtf(self, t, pos):
        """The sum-frequency 6-vectors of the owned bodies (world frame, at the body reference) at time t and positions pos; zeros
        with mode 0, without a table, and without wave components."""
        a = _arr(pos, 3 * self.N)
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_compute_sum_qtf(self.ctx, float(t), _dp(a), _dp(out)))
        return out

    def sum_qtf_begin(self, t, pos):
        a = _arr(pos, 3 * self.N)
        self._chk(self.lib.hc_sum_qtf_begin(self.ctx, float(t), _dp(a)))

    def sum_qtf_end(self):
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_sum_qtf_end(self.ctx, _dp(out)))
        return out

    def sum_qtf(self):
        """The sum-frequency term of the last step() (zeros when the mode is 0 or no table is set)."""
        m = self.__dict__.get("_sum_last")
        return np.zeros(self.D_local) if m is None or not self._sum_on() else m.copy()

    # -- state-space radiation by modal recursion (an extension beyond the reference) --
    def set_radiation_modes(self, b, modes):
        """Replaces the radiation modes of body b (0-based): an iterable of (row 0..5, col 0..D-1, lambda, rho) with complex pole
        (Re < 0) and residue in the units of the K given to set_body; an empty list clears them.  Once a body carries modes, step()
        returns total - modal radiation term: the term is independent of the convolution, so a modes-only caller gives the body a
        zero IRF (set_zero_rirf).  See hc_set_radiation_modes in include/hydrochrono_amd.h."""
        modes = list(modes)
        raw = (capi.RadiationMode * max(1, len(modes)))()
        for k, (row, col, lam, rho) in enumerate(modes):
            lam, rho = complex(lam), complex(rho)
            raw[k] = capi.RadiationMode(int(row), int(col), lam.real, lam.imag, rho.real, rho.imag)
        self._chk(self.lib.hc_set_radiation_modes(self.ctx, int(b), raw, len(modes)))
        counts = self.__dict__.setdefault("_radm_counts", {})
        counts[int(b)] = len(modes)
        self._radm_any = any(counts.values())

    def set_radiation_state_space(self, b, A, B, C):
        """The modes of body b from state-space models: A, B, C nested [6][D] lists (or object arrays) holding per pair an (n, n)
        matrix, an n-vector and an n-vector of any order n (None or an empty A: no model on that pair), K(tau) = C exp(A tau) B.
        Converted on the host (radiation_modes.state_space_to_modes); a defective or unstable A is refused."""
        from .radiation_modes import state_space_pairs_to_modes
        self.set_radiation_modes(b, state_space_pairs_to_modes(A, B, C, self.D))

    def radiation_mode_count(self, b):
        n = C.c_int()
        self._chk(self.lib.hc_get_radiation_mode_count(self.ctx, int(b), C.byref(n)))
        return n.value

    def set_radiation_modes_depth(self, depth):
        """Snapshots of the modal state kept for steps back in time: 2 .. 64, default 4."""
        self._chk(self.lib.hc_set_radiation_modes_depth(self.ctx, int(depth)))

    def reset_radiation_modes(self):
        self._chk(self.lib.hc_reset_radiation_modes(self.ctx))

    def radiation_modes_irf(self, b, tau):
        """K [6][D][n] = sum Re[rho exp(lambda tau)] of body b's modes, without the rho factor: what a fit is checked against."""
        tau = _arr(tau)
        K = np.empty((6, self.D, tau.size))
        self._chk(self.lib.hc_get_radiation_modes_irf(self.ctx, int(b), tau.size, _dp(tau), _dp(K.reshape(-1))))
        return K

    def set_zero_rirf(self, b, dt=0.05):
        """A zero radiation IRF of two samples for body b (before finalize): for a caller whose radiation comes from the modes alone.
        Every body of a system needs the same dt."""
        t = np.array([0.0, float(dt)])
        K = np.zeros(6 * self.D * 2)
        self._chk(self.lib.hc_set_rirf(self.ctx, int(b), _dp(t), 2, _dp(K)))

    def compute_radiation_modes(self, t, linvel, angvel):
        """Advances the modal state to time t with the velocities given and returns the modal radiation term of the owned bodies
        (sign and meaning of compute_radiation); zeros at the first call and without modes."""
        lv, av = _arr(linvel, 3 * self.N), _arr(angvel, 3 * self.N)
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_compute_radiation_modes(self.ctx, float(t), _dp(lv), _dp(av), _dp(out)))
        return out

    def radiation_modes_begin(self, t, linvel, angvel):
        lv, av = _arr(linvel, 3 * self.N), _arr(angvel, 3 * self.N)
        self._chk(self.lib.hc_radiation_modes_begin(self.ctx, float(t), _dp(lv), _dp(av)))

    def radiation_modes_end(self):
        out = np.empty(self.D_local)
        self._chk(self.lib.hc_radiation_modes_end(self.ctx, _dp(out)))
        return out

    def radiation_modes(self):
        """The modal radiation term of the last step() (zeros when no body carries modes)."""
        m = self.__dict__.get("_radm_last")
        return np.zeros(self.D_local) if m is None or not self.__dict__.get("_radm_any") else m.copy()


def wave_spreading_directions(nf, heading, s=0.0, n_bins=15, seed=1, lib=None):
    """hc_wave_spreading_directions: nf equal-energy directions of the cos-2s spreading about `heading` (no context needed)."""
    lib = lib or capi.load()
    th = np.empty(int(nf))
    rc = lib.hc_wave_spreading_directions(int(nf), float(heading), float(s), int(n_bins), int(seed), _dp(th))
    if rc != capi.HC_OK:
        raise HydroError(rc, "hc_wave_spreading_directions: bad arguments")
    return th


def triangles_to_panels(triangles):
    """Centroids and area vectors of triangles [n][3][3]."""
    tri = np.ascontiguousarray(triangles, dtype=np.float64).reshape(-1, 3, 3)
    c = (tri[:, 0] + tri[:, 1] + tri[:, 2]) / 3.0
    s = 0.5 * np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return c, s


def _compose_nonlinear(total, nl, mode, counts, b0, b1):
    """total - hs_lin + buoy (+ fk in mode 2) on the six rows of every body of [b0, b1) that carries panels; the other rows untouched."""
    buoy, fk, hs_lin = nl
    out = total.copy()
    for b, n in counts.items():
        if n and b0 <= b < b1:
            r = slice(6 * (b - b0), 6 * (b - b0) + 6)
            out[r] = total[r] - hs_lin[r] + buoy[r]
            if mode == 2:
                out[r] = out[r] + fk[r]
    return out


class _SideTerm(NamedTuple):
    """A term that runs on a lane of its own beside the step: its C begin / end pair, which of (pos, rpy, linvel, angvel) the begin
    takes, how many D_local arrays the end fills, whether it is on (asked of a HydroForces), where the last value is kept, and how
    it joins the total: compose(out, x, cfg, b0, b1), cfg the HydroForces that holds the nonlinear mode and the panel counts."""
    name: str
    begin: str
    end: str
    slots: tuple
    nout: int
    on: Callable
    last: str
    compose: Callable


# the order of the rows is the order of the begins, of the ends and of the composition
_SIDE_TERMS = (
    _SideTerm("nonlinear", "hc_nonlinear_begin", "hc_nonlinear_end", (0, 1), 3, lambda h: h._nonlinear_on(), "_nonlinear_last",
              lambda out, x, cfg, b0, b1: _compose_nonlinear(out, x, cfg._nonlinear_mode, cfg._panel_counts, b0, b1)),
    _SideTerm("morison", "hc_morison_begin", "hc_morison_end", (0, 1, 2, 3), 1, lambda h: h.__dict__.get("_morison_any"), "_morison_last",
              lambda out, x, *_: out + x),
    _SideTerm("drift", "hc_drift_begin", "hc_drift_end", (0,), 1, lambda h: h._drift_on(), "_drift_last", lambda out, x, *_: out + x),
    _SideTerm("sum", "hc_sum_qtf_begin", "hc_sum_qtf_end", (0,), 1, lambda h: h._sum_on(), "_sum_last", lambda out, x, *_: out + x),
    _SideTerm("radm", "hc_radiation_modes_begin", "hc_radiation_modes_end", (2, 3), 1, lambda h: h.__dict__.get("_radm_any"), "_radm_last",
              lambda out, x, *_: out - x),
)
_NONLINEAR, _MORISON, _DRIFT, _SUM, _RADM = _SIDE_TERMS


def _side_error(lib, ctx, rc):
    return HydroError(rc, lib.hc_last_error(ctx).decode())


def _side_drop(lib, ctxs, term):
    """Ends `term` on the contexts (ctx, first row, rows) into scratch arrays: nothing stays pending."""
    end = getattr(lib, term.end)
    for ctx, _, n in ctxs:
        end(ctx, *(_dp(np.empty(n)) for _ in range(term.nout)))


def _side_begin(lib, ctxs, term, t, a):
    """Begins `term` on every context with the arrays a[slot]; a refusal ends it on the contexts before and is raised."""
    begin = getattr(lib, term.begin)
    args = [_dp(a[s]) for s in term.slots]
    for g, (ctx, _, _) in enumerate(ctxs):
        rc = begin(ctx, float(t), *args)
        if rc:
            err = _side_error(lib, ctx, rc)
            _side_drop(lib, ctxs[:g], term)
            raise err


def _side_end(lib, ctxs, term, D):
    """Ends `term` on every context, each into its rows of arrays of D: (the array, or the tuple of them where the term has several;
    the error of the first context that refused, or None)."""
    end = getattr(lib, term.end)
    val = tuple(np.empty(D) for _ in range(term.nout))
    err = None
    for ctx, row, n in ctxs:
        rc = end(ctx, *(_dp(x[row:row + n]) for x in val))
        if rc and err is None:
            err = _side_error(lib, ctx, rc)
    return (val if term.nout > 1 else val[0]), err


def _step_with_side_terms(owner, cfg, ctxs, on, step, t, a, out, b0, b1):
    """The step with the terms of _SIDE_TERMS whose flag in `on` is set, on the contexts (ctx, first row, rows) of one system:
    begin each term on every context in table order -- a refused begin ends what was begun, and is raised; step() -> status, which
    fills `out`; end every term on every context, whatever the step answered; raise the step's error, else the first end's (table
    order, then context order); then, and only then, keep the values in owner.<term.last> and compose them in table order."""
    lib = owner.lib
    terms = [term for term, flag in zip(_SIDE_TERMS, on) if flag]
    for k, term in enumerate(terms):
        try:
            _side_begin(lib, ctxs, term, t, a)
        except HydroError:
            for earlier in terms[:k]:
                _side_drop(lib, ctxs, earlier)
            raise
    rc = step()
    err = _side_error(lib, ctxs[0][0], rc) if rc else None
    vals = []
    for term in terms:
        val, end_err = _side_end(lib, ctxs, term, out.size)
        vals.append(val)
        err = err or end_err
    if err:
        raise err
    for term, val in zip(terms, vals):
        setattr(owner, term.last, val)
        out = term.compose(out, val, cfg, b0, b1)
    return out


def read_eta_file(path):
    """IrregularWaves::ReadEtaFromFile: the `time : eta` lines of an eta file as (t, eta); HydroError with the reference's message
    on a file that cannot be opened or a line that cannot be parsed."""
    lib = capi.load()
    path = str(path).encode()
    n = C.c_int()
    rc = lib.hc_read_eta_file(path, None, None, 0, C.byref(n))
    if rc == capi.HC_OK:
        t, eta = np.empty(n.value), np.empty(n.value)
        rc = lib.hc_read_eta_file(path, _dp(t), _dp(eta), n.value, C.byref(n))
    if rc != capi.HC_OK:
        raise HydroError(rc, lib.hc_last_error(None).decode())
    return t, eta


class HydroGroup:
    """G row-sharded contexts of ONE coupled N-body system driven by one host process through hc_step_multi /
    hc_added_mass_mv_multi (drop-in variant: host holds all state -> a state store per GPU -> host gather).
    `shards` are HydroForces objects created with body_range=... that together cover bodies [0, N)."""

    def __init__(self, shards):
        self.shards = list(shards)
        self.N = self.shards[0].N
        self.D = 6 * self.N
        self.lib = self.shards[0].lib
        covered = sorted((h.b0, h.b1) for h in self.shards)
        if covered[0][0] != 0 or covered[-1][1] != self.N or any(a[1] != b[0] for a, b in zip(covered, covered[1:])):
            raise ValueError("the shards do not partition bodies [0, N)")
        self._ctxs = (C.c_void_p * len(self.shards))(*[h.ctx for h in self.shards])
        self._side_ctxs = [(h.ctx, 6 * h.b0, h.D_local) for h in self.shards]  # (context, first row, rows) as the side-term driver takes them
        self._step =C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)(
            ("hc_step_multi", self.lib))

    @classmethod
    def from_case(cls, case, n_shards, devices=None):
        from .parallel_split import body_shard
        devices = devices or [0] * n_shards
        return cls([HydroForces.from_case(case, device=devices[g], body_range=body_shard(case["N"], n_shards, g)) for g in range(n_shards)])

    def __getattr__(self, name):
        # configuration calls (add_waves_*, set_lookahead, set_history, ...) go to every shard
        if name.startswith(("add_waves", "set_", "reset_", "enable_")):
            def fan_out(*a, **k):
                for h in self.shards:
                    getattr(h, name)(*a, **k)
            return fan_out
        raise AttributeError(name)

    def step(self, t, pos, rpy, linvel, angvel):
        n3 = 3 * self.N
        a = [_arr(x, n3) for x in (pos, rpy, linvel, angvel)]
        out = np.empty(self.D)

        def step():
            return self._step(self._ctxs, len(self.shards), t, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, out.ctypes.data)
        return _step_with_side_terms(self, self.shards[0], self._side_ctxs, [self._side_on(term) for term in _SIDE_TERMS], step, t, a, out,
                                     0, self.N)

    # -- the terms beside the step (_SIDE_TERMS).  Every shard holds the lists, tables and modes of all bodies and computes the rows of
    # its own: a term is begun on every shard, then ended on every shard, each into its rows --
    def _side_on(self, term):
        # the first shard answers for all; the element lists are asked of each
        return any(term.on(h) for h in self.shards) if term is _MORISON else term.on(self.shards[0])

    def _begin_term(self, term, t, *arrays):
        _side_begin(self.lib, self._side_ctxs, term, t, dict(zip(term.slots, (_arr(x, 3 * self.N) for x in arrays))))

    def _end_term(self, term):
        val, err = _side_end(self.lib, self._side_ctxs, term, self.D)
        if err:
            raise err
        return val

    def _compute_term(self, term, t, *arrays):
        self._begin_term(term, t, *arrays)
        return self._end_term(term)

    def _last_term(self, term):
        """The term's value in the last step(); zeros before the first one and while the term is off."""
        m = self.__dict__.get(term.last)
        if m is None or not self._side_on(term):
            m = tuple(np.zeros(self.D) for _ in range(term.nout))
            return m if term.nout > 1 else m[0]
        return tuple(x.copy() for x in m) if term.nout > 1 else m.copy()

    def compute_drift(self, t, pos):
        return self._compute_term(_DRIFT, t, pos)

    def drift(self):
        return self._last_term(_DRIFT)

    def drift_qtf_size(self, b):
        return self.shards[0].drift_qtf_size(b)

    def drift_qtf_headings(self, b):
        return self.shards[0].drift_qtf_headings(b)

    def compute_sum_qtf(self, t, pos):
        return self._compute_term(_SUM, t, pos)

    def sum_qtf_begin(self, t, pos):
        self._begin_term(_SUM, t, pos)

    def sum_qtf_end(self):
        return self._end_term(_SUM)

    def sum_qtf(self):
        return self._last_term(_SUM)

    def sum_qtf_size(self, b):
        return self.shards[0].sum_qtf_size(b)

    def sum_qtf_headings(self, b):
        return self.shards[0].sum_qtf_headings(b)

    def compute_radiation_modes(self, t, linvel, angvel):
        return self._compute_term(_RADM, t, linvel, angvel)

    def radiation_modes(self):
        return self._last_term(_RADM)

    def radiation_modes_irf(self, b, tau):
        return self.shards[0].radiation_modes_irf(b, tau)

    def radiation_mode_count(self, b):
        return self.shards[0].radiation_mode_count(b)

    def surface_panel_count(self, b):
        return self.shards[0].surface_panel_count(b)

    def surface_triangle_count(self, b):
        return self.shards[0].surface_triangle_count(b)

    def compute_nonlinear(self, t, pos, rpy):
        return self._compute_term(_NONLINEAR, t, pos, rpy)

    def nonlinear(self):
        return self._last_term(_NONLINEAR)

    def compute_morison(self, t, pos, rpy, linvel, angvel):
        return self._compute_term(_MORISON, t, pos, rpy, linvel, angvel)

    def morison(self):
        return self._last_term(_MORISON)

    def nonlinear_second_order(self):
        return self.shards[0].nonlinear_second_order()

    def nonlinear_second_order_directional(self):
        return self.shards[0].nonlinear_second_order_directional()

    def nonlinear_point_count(self, b):
        return self.shards[0].nonlinear_point_count(b)

    def nonlinear_increments(self, b):
        # the shard that owns the body answers
        for h in self.shards:
            if h.b0 <= int(b) < h.b1:
                return h.nonlinear_increments(b)
        raise IndexError(f"body {b} out of range")

    def morison_second_order(self):
        return self.shards[0].morison_second_order()

    def morison_second_order_directional(self):
        return self.shards[0].morison_second_order_directional()

    def morison_member_count(self, b):
        return self.shards[0].morison_member_count(b)

    def morison_members_second_order(self):
        return self.shards[0].morison_members_second_order()

    def morison_member_increments(self, b):
        # the shard that owns the body answers
        for h in self.shards:
            if h.b0 <= int(b) < h.b1:
                return h.morison_member_increments(b)
        raise IndexError(f"body {b} out of range")

    def morison_member_forces(self, b):
        # the shard that owns the body answers
        for h in self.shards:
            if h.b0 <= int(b) < h.b1:
                return h.morison_member_forces(b)
        raise IndexError(f"body {b} out of range")

    def morison_increments(self, b):
        # the shard that owns the body answers
        for h in self.shards:
            if h.b0 <= int(b) < h.b1:
                return h.morison_increments(b)
        raise IndexError(f"body {b} out of range")

    def morison_member_added_mass_coefficients(self, b):
        return self.shards[0].morison_member_added_mass_coefficients(b)

    def morison_added_mass(self, body=None):
        # the shard that owns a body answers; body=None: (N, 6, 6), the shards' blocks in body order
        if body is None:
            return np.concatenate([h.morison_added_mass() for h in sorted(self.shards, key=lambda h: h.b0)])
        for h in self.shards:
            if h.b0 <= int(body) < h.b1:
                return h.morison_added_mass(body)
        raise IndexError(f"body {body} out of range")

    def morison_member_added_mass(self, b):
        for h in self.shards:
            if h.b0 <= int(b) < h.b1:
                return h.morison_member_added_mass(b)
        raise IndexError(f"body {b} out of range")

    def morison_added_mass_force(self, linacc, angacc):
        return np.concatenate([h.morison_added_mass_force(linacc, angacc) for h in sorted(self.shards, key=lambda h: h.b0)])

    def add_waves_irregular_eta(self, t, eta, simulation_dt, num_bodies=None):
        # every shard takes the whole record
        for h in self.shards:
            h.add_waves_irregular_eta(t, eta, simulation_dt, num_bodies)

    def set_eta_record_components(self, f_min, f_max, max_components=0):
        # every shard analyses the whole record and gets the same bits
        for h in self.shards:
            h.set_eta_record_components(f_min, f_max, max_components)

    def clear_eta_record_components(self):
        for h in self.shards:
            h.clear_eta_record_components()

    def eta_record_components(self):
        return self.shards[0].eta_record_components()

    def components(self):
        parts = [h.components() for h in sorted(self.shards, key=lambda h: h.b0)]
        return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))

    def wave_directions(self):
        return self.shards[0].wave_directions()

    def set_wave_spreading(self, heading, s=0.0, n_bins=15, seed=1):
        """As HydroForces.set_wave_spreading: the directions are generated once, set on every shard and returned."""
        th = wave_spreading_directions(self.shards[0].wave_component_count(), heading, s, n_bins, seed, lib=self.lib)
        for h in self.shards:
            h.set_wave_directions(th)
        return th

    def wave_kinematics(self, points, times, **opts):
        # every shard holds the whole wave model and answers with the same bits
        return self.shards[0].wave_kinematics(points, times, **opts)

    def wave_kinematics2(self, points, times, **opts):
        # every shard holds the whole wave model: any of them answers (hc_wave_kinematics2: same bits from each)
        return self.shards[0].wave_kinematics2(points, times, **opts)

    def wave_pair_tables(self, **opts):
        return self.shards[0].wave_pair_tables(**opts)

    def added_mass_mv(self, R, w, c):
        R = _arr(R).copy()
        w = _arr(w)
        rc = self.lib.hc_added_mass_mv_multi(self._ctxs, len(self.shards), _dp(w), float(c), _dp(R), R.size)
        if rc:
            raise HydroError(rc, self.lib.hc_last_error(self.shards[0].ctx).decode())
        return R

    def close(self):
        for h in self.shards:
            h.close()
