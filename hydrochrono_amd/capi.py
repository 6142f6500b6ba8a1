"""ctypes binding of the C ABI in include/hydrochrono_amd.h (libhydrochrono_amd.so).

This module only declares signatures and loads the library.  It fails loudly if the HIP library is missing:
the hydro-force path has no CPU fallback.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libhydrochrono_amd.so")
# the same sources built with -DHC_TUNING (hydrochrono_amd/build.py): reads the sweep / A-B / fault-injection switches of
# csrc/hc_internal.hpp (HC_TUNE_INT) and holds the kernel variants that were measured and not taken; loaded by tests and probes only
TUNING_LIB_PATH = os.path.join(_PKG, "lib", "libhydrochrono_amd_tuning.so")

HC_OK, HC_ERR_RUNTIME, HC_ERR_OUT_OF_RANGE, HC_ERR_INVALID, HC_ERR_DEVICE, HC_ERR_UNSUPPORTED = range(6)

c_double_p = C.POINTER(C.c_double)
c_int_p = C.POINTER(C.c_int)


class IrregularWaveParams(C.Structure):
    """hc_irregular_wave_params == IrregularWaveParams (include/hydroc/wave_types.h:277-292)."""
    _fields_ = [("num_bodies", C.c_int), ("simulation_dt", C.c_double), ("simulation_duration", C.c_double),
                ("ramp_duration", C.c_double), ("wave_height", C.c_double), ("wave_period", C.c_double),
                ("frequency_min", C.c_double), ("frequency_max", C.c_double), ("nfrequencies", C.c_double),
                ("peak_enhancement_factor", C.c_double), ("is_normalized", C.c_int), ("seed", C.c_int)]


class TaperedDirectOptions(C.Structure):
    """hc_tapered_direct_options == TestHydro::TaperedDirectOptions (include/hydroc/hydro_forces.h:246-259)."""
    _fields_ = [("smoothing", C.c_int), ("window_length", C.c_int), ("rirf_end_time", C.c_double),
                ("taper_start_percent", C.c_double), ("taper_end_percent", C.c_double),
                ("taper_final_amplitude", C.c_double), ("export_plot_csv", C.c_int)]


class WaveKinematicsOpts(C.Structure):
    """hc_wave_kinematics_opts: WaveBase::mwl_, RegularWave::regular_wave_phase_, IrregularWaveParams::wave_stretching_."""
    _fields_ = [("mwl", C.c_double), ("regular_phase", C.c_double), ("wave_stretching", C.c_int)]


class WaveKinematics2Opts(C.Structure):
    """hc_wave_kinematics2_opts: mwl and regular phase as above, the difference- and sum-frequency cut-offs [rad/s], the ramp switch."""
    _fields_ = [("mwl", C.c_double), ("regular_phase", C.c_double), ("diff_lo", C.c_double), ("diff_hi", C.c_double),
                ("sum_lo", C.c_double), ("sum_hi", C.c_double), ("apply_ramp", C.c_int)]


class MorisonElement(C.Structure):
    """hc_morison_element: position in the body frame, Cd_i A_i and Cm_i V per body axis."""
    _fields_ = [("r", C.c_double * 3), ("cd_area", C.c_double * 3), ("cm_vol", C.c_double * 3)]


class MorisonMember(C.Structure):
    """hc_morison_member: end points in the body frame, the diameter at each, Cd, Cm, segments (88 bytes)."""
    _fields_ = [("r0", C.c_double * 3), ("r1", C.c_double * 3), ("d0", C.c_double), ("d1", C.c_double), ("cd", C.c_double),
                ("cm", C.c_double), ("n_seg", C.c_int)]


class SurfacePanel(C.Structure):
    """hc_surface_panel: centroid and area vector (outward normal times area) in the body frame."""
    _fields_ = [("c", C.c_double * 3), ("s", C.c_double * 3)]


class RadiationMode(C.Structure):
    """hc_radiation_mode: row 0..5 of the body, column 0..D-1, complex pole and residue."""
    _fields_ = [("row", C.c_int), ("col", C.c_int), ("lambda_re", C.c_double), ("lambda_im", C.c_double),
                ("rho_re", C.c_double), ("rho_im", C.c_double)]


class ProfileStats(C.Structure):
    _fields_ = [("hydrostatics_seconds", C.c_double), ("radiation_seconds", C.c_double), ("waves_seconds", C.c_double),
                ("hydrostatics_calls", C.c_int), ("radiation_calls", C.c_int), ("waves_calls", C.c_int),
                ("conv_kernel_seconds", C.c_double), ("conv_kernel_launches", C.c_longlong),
                ("conv_kernel_bytes", C.c_double), ("block_kernel_seconds", C.c_double),
                ("block_kernel_launches", C.c_longlong), ("block_kernel_bytes", C.c_double),
                ("block_kernel_bytes_once", C.c_double),
                ("step_kernel_seconds", C.c_double), ("step_kernel_launches", C.c_longlong),
                ("scatter_kernel_seconds", C.c_double), ("scatter_kernel_launches", C.c_longlong),
                ("direct_dispatches", C.c_longlong), ("hip_launches", C.c_longlong), ("history_rewinds", C.c_longlong),
                ("mini_pass_seconds", C.c_double), ("mini_pass_launches", C.c_longlong), ("queue_parkings", C.c_longlong),
                ("ahead_pass_slices", C.c_longlong), ("ahead_blocks", C.c_longlong),
                ("pass_lane_launches", C.c_longlong),
                ("multi_doorbell_offset_last", C.c_double), ("multi_doorbell_offset_sum", C.c_double), ("multi_calls", C.c_longlong),
                ("slot_state_steps", C.c_longlong), ("wide_fused_steps", C.c_longlong),
                ("schedule_blocks_ahead", C.c_longlong), ("schedule_blocks_at_start", C.c_longlong), ("ring_grows_for_pass", C.c_longlong),
                ("hot_steps", C.c_longlong), ("tail_launches", C.c_longlong), ("tail_seconds", C.c_double),
                ("tail_bytes", C.c_double), ("tail_blocks", C.c_longlong)]


class InitStats(C.Structure):
    _fields_ = [("h5_read_seconds", C.c_double), ("h5_read_bytes", C.c_double), ("rirf_h2d_seconds", C.c_double), ("rirf_h2d_bytes", C.c_double),
                ("rirf_relayout_seconds", C.c_double), ("rirf_relayout_bytes", C.c_double), ("finalize_seconds", C.c_double),
                ("direct_setup_seconds", C.c_double), ("wave_resample_seconds", C.c_double), ("wave_spectrum_seconds", C.c_double),
                ("wave_eta_seconds", C.c_double), ("wave_eta_samples", C.c_longlong), ("wave_eta_components", C.c_longlong),
                ("wave_eta_mode", C.c_int), ("pad_", C.c_int), ("wave_upload_seconds", C.c_double), ("wave_upload_bytes", C.c_double),
                ("wave_total_seconds", C.c_double), ("taper_seconds", C.c_double), ("taper_bytes", C.c_double),
                ("synth_seconds", C.c_double), ("synth_bytes", C.c_double)]


# name -> (restype, argtypes); every symbol include/hydrochrono_amd.h declares
SIGNATURES = {
    "hc_version": (C.c_char_p, []),
    "hc_device_count": (C.c_int, []),
    "hc_device_local_cpus": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "hc_bind_thread_to_device": (C.c_int, [C.c_int]),
    "hc_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "hc_create_sharded": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "hc_destroy": (None, [C.c_void_p]),
    "hc_last_error": (C.c_char_p, [C.c_void_p]),
    "hc_set_simulation_parameters": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double]),
    "hc_set_body_properties": (C.c_int, [C.c_void_p, C.c_int, C.c_double, c_double_p, c_double_p]),
    "hc_set_hydrostatic_stiffness": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_set_added_mass_inf": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_set_rirf": (C.c_int, [C.c_void_p, C.c_int, c_double_p, C.c_int, c_double_p]),
    "hc_set_excitation_rao": (C.c_int, [C.c_void_p, C.c_int, c_double_p, C.c_int, c_double_p, c_double_p]),
    "hc_set_excitation_irf": (C.c_int, [C.c_void_p, C.c_int, c_double_p, C.c_int, c_double_p]),
    "hc_load_bemio_h5": (C.c_int, [C.c_void_p, C.c_char_p]),
    "hc_finalize": (C.c_int, [C.c_void_p]),
    "hc_set_gravity": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_set_wave_none": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_set_wave_regular": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double]),
    "hc_irregular_wave_params_default": (None, [C.POINTER(IrregularWaveParams)]),
    "hc_set_wave_irregular": (C.c_int, [C.c_void_p, C.POINTER(IrregularWaveParams)]),
    "hc_set_wave_irregular_eta": (C.c_int, [C.c_void_p, C.POINTER(IrregularWaveParams), c_double_p, c_double_p, C.c_int]),
    "hc_read_eta_file": (C.c_int, [C.c_char_p, c_double_p, c_double_p, C.c_int, c_int_p]),
    "hc_set_eta_record_components": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "hc_clear_eta_record_components": (C.c_int, [C.c_void_p]),
    "hc_get_eta_record_components": (C.c_int, [C.c_void_p, c_int_p, c_int_p] + [c_double_p] * 7),
    "hc_set_eta_synthesis": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_set_wave_irregular_spectral": (C.c_int, [C.c_void_p, C.POINTER(IrregularWaveParams)]),
    "hc_set_convolution_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_tapered_direct_options_default": (None, [C.POINTER(TaperedDirectOptions)]),
    "hc_set_tapered_direct_options": (C.c_int, [C.c_void_p, C.POINTER(TaperedDirectOptions)]),
    "hc_set_diagnostics_output_directory": (C.c_int, [C.c_void_p, C.c_char_p]),
    "hc_get_shard": (C.c_int, [C.c_void_p, c_int_p, c_int_p]),
    "hc_get_excitation_irf_size": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_step": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_step_begin": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_step_end": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_step_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_added_mass_mv_multi": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, c_double_p, C.c_double, c_double_p, C.c_int]),
    "hc_set_result_buffer": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "hc_step_sequence": (C.c_int, [C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "hc_wait_result_buffer": (C.c_int, [C.c_void_p, C.c_int, C.c_ulonglong, c_double_p, C.c_double]),
    "hc_step_device": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "hc_get_force_components": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "hc_compute_radiation": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, c_double_p]),
    "hc_compute_hydrostatics": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "hc_compute_waves": (C.c_int, [C.c_void_p, C.c_double, c_double_p]),
    "hc_set_lookahead": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_set_pass_schedule": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "hc_set_radiation_tail": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_get_schedule": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "hc_direct_dispatch_active": (C.c_int, [C.c_void_p]),
    "hc_dispatch_mode_reason": (C.c_char_p, [C.c_void_p]),
    "hc_reset_history": (C.c_int, [C.c_void_p]),
    "hc_set_history": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p]),
    "hc_get_history": (C.c_int, [C.c_void_p, c_int_p, c_double_p, c_double_p]),
    "hc_added_mass_matrix": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_added_mass_mv": (C.c_int, [C.c_void_p, c_double_p, C.c_double, c_double_p, C.c_int]),
    "hc_enable_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_get_profile": (C.c_int, [C.c_void_p, C.POINTER(ProfileStats)]),
    "hc_get_init_stats": (C.c_int, [C.c_void_p, C.POINTER(InitStats)]),
    "hc_reset_profile": (C.c_int, [C.c_void_p]),
    "hc_get_sizes": (C.c_int, [C.c_void_p] + [c_int_p] * 8),
    "hc_get_rirf_width": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_get_rirf_effective": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_get_rirf_value": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, c_double_p]),
    "hc_step_many": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    "hc_h5_read": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]),
    "hc_h5_free": (None, [C.c_void_p]),
    "hc_h5_get_sizes": (C.c_int, [C.c_void_p, c_int_p, c_double_p, c_double_p, c_double_p, C.c_int, c_int_p, c_int_p, c_int_p]),
    "hc_h5_get_body": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_h5_get_rirf": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_h5_get_excitation_rao": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p]),
    "hc_h5_get_excitation_irf": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p]),
    "hc_get_excitation_irf_resampled": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p]),
    "hc_get_spectrum": (C.c_int, [C.c_void_p] + [c_double_p] * 5),
    "hc_get_eta_table": (C.c_int, [C.c_void_p, c_double_p, c_double_p]),
    "hc_export_irregular_inputs_h5": (C.c_int, [C.c_void_p, C.c_char_p]),
    "hc_get_regular_coeffs": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "hc_get_simulation_parameters": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "hc_wave_kinematics_opts_default": (None, [C.POINTER(WaveKinematicsOpts)]),
    "hc_wave_kinematics": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematicsOpts), C.c_int, c_double_p, C.c_int, c_double_p,
                                     c_double_p, c_double_p, c_double_p]),
    "hc_set_morison_elements": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(MorisonElement), C.c_int]),
    "hc_set_wave_directions": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_get_wave_directions": (C.c_int, [C.c_void_p, c_int_p, c_double_p]),
    "hc_set_excitation_rao_headings": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, C.c_int, c_double_p, c_double_p]),
    "hc_get_excitation_rao_headings_size": (C.c_int, [C.c_void_p, C.c_int, c_int_p, c_int_p]),
    "hc_wave_spreading_directions": (C.c_int, [C.c_int, C.c_double, C.c_double, C.c_int, C.c_ulonglong, c_double_p]),
    "hc_get_morison_count": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_morison_options": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematicsOpts)]),
    "hc_morison_begin": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_morison_end": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_compute_morison": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_set_morison_second_order": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]),
    "hc_get_morison_second_order": (C.c_int, [C.c_void_p, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    "hc_set_morison_second_order_directional": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_get_morison_second_order_directional": (C.c_int, [C.c_void_p, c_int_p]),
    "hc_get_morison_increments": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_set_morison_members": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(MorisonMember), C.c_int]),
    "hc_get_morison_member_count": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_get_morison_member_forces": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_set_morison_member_added_mass": (C.c_int, [C.c_void_p, C.c_int, c_double_p, C.c_int]),
    "hc_get_morison_member_added_mass_coefficients": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_get_morison_added_mass": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_get_morison_member_added_mass": (C.c_int, [C.c_void_p, C.c_int, c_double_p]),
    "hc_set_morison_members_second_order": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_get_morison_members_second_order": (C.c_int, [C.c_void_p, c_int_p]),
    "hc_get_morison_member_increment_counts": (C.c_int, [C.c_void_p, C.c_int, c_int_p, c_int_p]),
    "hc_get_morison_member_node_increments": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p]),
    "hc_get_morison_member_point_increments": (C.c_int, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_set_surface_panels": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SurfacePanel), C.c_int]),
    "hc_get_surface_panel_count": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_surface_triangles": (C.c_int, [C.c_void_p, C.c_int, c_double_p, C.c_int]),
    "hc_get_surface_triangle_count": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_nonlinear_options": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematicsOpts)]),
    "hc_nonlinear_begin": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p]),
    "hc_nonlinear_end": (C.c_int, [C.c_void_p, c_double_p, c_double_p, c_double_p]),
    "hc_compute_nonlinear": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_set_nonlinear_second_order": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int]),
    "hc_get_nonlinear_second_order": (C.c_int, [C.c_void_p, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    "hc_set_nonlinear_second_order_directional": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_get_nonlinear_second_order_directional": (C.c_int, [C.c_void_p, c_int_p]),
    "hc_get_nonlinear_point_count": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_get_nonlinear_increments": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    "hc_set_drift_qtf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    "hc_get_drift_qtf_size": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_drift_qtf_headings": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p]),
    "hc_get_drift_qtf_headings": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_drift_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_get_drift_mode": (C.c_int, [C.c_void_p, c_int_p]),
    "hc_set_drift_options": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematicsOpts)]),
    "hc_drift_begin": (C.c_int, [C.c_void_p, C.c_double, c_double_p]),
    "hc_drift_end": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_compute_drift": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p]),
    "hc_set_sum_qtf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p]),
    "hc_get_sum_qtf_size": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_sum_qtf_headings": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p]),
    "hc_get_sum_qtf_headings": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_sum_mode": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_get_sum_mode": (C.c_int, [C.c_void_p, c_int_p]),
    "hc_set_sum_options": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematicsOpts)]),
    "hc_sum_qtf_begin": (C.c_int, [C.c_void_p, C.c_double, c_double_p]),
    "hc_sum_qtf_end": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_compute_sum_qtf": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p]),
    "hc_wave_kinematics2_opts_default": (None, [C.POINTER(WaveKinematics2Opts)]),
    "hc_wave_kinematics2": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematics2Opts), C.c_int, c_double_p, C.c_int, c_double_p,
                                      c_double_p, c_double_p, c_double_p]),
    "hc_wave_kinematics2_pair_tables": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematics2Opts), c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_wave_kinematics2_dir": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematics2Opts), C.c_int, c_double_p, C.c_int, c_double_p,
                                          c_double_p, c_double_p, c_double_p]),
    "hc_wave_kinematics2_dir_pair_tables": (C.c_int, [C.c_void_p, C.POINTER(WaveKinematics2Opts), c_double_p, c_double_p, c_double_p, c_double_p]),
    "hc_set_radiation_modes": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(RadiationMode), C.c_int]),
    "hc_get_radiation_mode_count": (C.c_int, [C.c_void_p, C.c_int, c_int_p]),
    "hc_set_radiation_modes_depth": (C.c_int, [C.c_void_p, C.c_int]),
    "hc_radiation_modes_begin": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p]),
    "hc_radiation_modes_end": (C.c_int, [C.c_void_p, c_double_p]),
    "hc_compute_radiation_modes": (C.c_int, [C.c_void_p, C.c_double, c_double_p, c_double_p, c_double_p]),
    "hc_reset_radiation_modes": (C.c_int, [C.c_void_p]),
    "hc_get_radiation_modes_irf": (C.c_int, [C.c_void_p, C.c_int, C.c_int, c_double_p, c_double_p]),
    "hc_synth_fill": (C.c_int, [C.c_void_p, C.c_ulonglong, C.c_int, C.c_double, C.c_int, C.c_double]),
}

# include/hydrochrono_amd_host.h
SIGNATURES.update({
    "hc_host_linspaced": (None, [C.c_int, C.c_double, C.c_double, c_double_p]),
    "hc_host_trapezoid_widths": (None, [c_double_p, C.c_int, c_double_p]),
    "hc_host_jonswap_spectrum_hz": (None, [c_double_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, c_double_p]),
    "hc_host_random_phases": (None, [C.c_int, C.c_int, c_double_p]),
    "hc_host_wave_number": (C.c_double, [C.c_double, C.c_double, C.c_double]),
    "hc_host_resample_irf": (C.c_int, [c_double_p, C.c_int, C.c_int, c_double_p]),
})

# include/hydrochrono_amd_yaml.h
SIGNATURES.update({
    "hc_yaml_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]),
    "hc_yaml_free": (None, [C.c_void_p]),
    "hc_yaml_num_bodies": (C.c_int, [C.c_void_p]),
    "hc_yaml_body_string": (C.c_char_p, [C.c_void_p, C.c_int, C.c_char_p]),
    "hc_yaml_body_number": (C.c_double, [C.c_void_p, C.c_int, C.c_char_p]),
    "hc_yaml_string": (C.c_char_p, [C.c_void_p, C.c_char_p]),
    "hc_yaml_number": (C.c_double, [C.c_void_p, C.c_char_p]),
    "hc_yaml_period_values": (C.c_int, [C.c_void_p, c_double_p, C.c_int]),
    "hc_create_from_hydro_yaml": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_double, C.c_double, C.c_double, C.c_int,
                                            C.POINTER(C.c_void_p), c_int_p, c_int_p, C.c_char_p, C.c_size_t]),
    "hc_create_from_hydro_yaml_sharded": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_double, C.c_double, C.c_double, c_int_p, C.c_int,
                                                    C.POINTER(C.c_void_p), c_int_p, c_int_p, C.c_char_p, C.c_size_t]),
})

_libs = {}        # flavour -> loaded library
_step_raws = {}   # flavour -> hc_step bound with integer arguments
_flavor = "tuning" if os.environ.get("HYDROCHRONO_AMD_FLAVOR", "release") == "tuning" else "release"  # (subprocesses of tests / sweeps)


def flavor():
    return _flavor


class use_flavor:
    """`with capi.use_flavor("tuning"):` -- objects created inside (HydroForces, ...) bind to libhydrochrono_amd_tuning.so and keep it
    for their lifetime; the release library stays the default outside.  Both may be loaded in one process: they share nothing but
    the HIP runtime (each is linked -Bsymbolic and loaded RTLD_LOCAL)."""

    def __init__(self, name):
        if name not in ("release", "tuning"):
            raise ValueError(name)
        self.name = name

    def __enter__(self):
        global _flavor
        self.prev, _flavor = _flavor, self.name
        return load()

    def __exit__(self, *exc):
        global _flavor
        _flavor = self.prev
        return False


def step_raw(lib=None):
    """hc_step bound with integer (address) arguments: skips the per-call ctypes pointer conversions."""
    lib = lib or load()
    fn = _step_raws.get(id(lib))
    if fn is None:
        proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
        fn = _step_raws[id(lib)] = proto(("hc_step", lib))
    return fn


def load(which=None):
    """Load libhydrochrono_amd.so (or, inside use_flavor("tuning") / with which="tuning", its tuning build); raises if it has not
    been built (no fallback)."""
    which = which or _flavor
    if which in _libs:
        return _libs[which]
    path = LIB_PATH if which == "release" else TUNING_LIB_PATH
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build the HIP extension first (python -m hydrochrono_amd.build, or "
            "__graft_entry__.build()).  The hydro-force path has no CPU fallback.")
    lib = C.CDLL(path, mode=C.RTLD_LOCAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _libs[which] = lib
    return lib
