// hc_wave_kin.hpp -- the per-component table of the wave kinematics, shared by the kernels that sum over it (hc_wave_kin.hip:
// wave_kinematics_kernel; hc_morison.hip: morison_items_kernel).  Built on the host once per wave model (hc_wave_kin.hip).
#pragma once
#include <vector>

struct hc_ctx;

namespace hc {

constexpr int kKinTile = 256;  // wave components staged in LDS per tile

// The per-component table, struct of arrays [kKinCols][nf].
enum KinCol {
    kKinAmp = 0,   // A
    kKinOmega,     // omega
    kKinK,         // wavenumber k
    kKinPhase,     // phi
    kKinWA,        // omega * A
    kKinW2A,       // omega * omega * A
    kKinInvSinh,   // 1 / sinh(k d) (finite-depth profile; 0 where the exponential profile applies)
    kKinDeep,      // 1: exponential profile (2 pi / k > d || k d > 500, per component as the reference tests it)
    kKinCols
};

// The table of the context's wave model (regular: one component with the caller's phase; irregular and spectral: the spectrum of
// the context, A_i = sqrt(2 S_i df_i) and w_i = 2 pi f_i as build_spectrum / the reference compute them; an imported eta record
// with components (hc_set_eta_record_components): the amplitudes of its analysis as they are).  Empty for NoWave and for an imported
// eta record without components (no spectrum).
std::vector<double> kin_table_host(const hc_ctx* c, double regular_phase);
// Some component in that table: a regular wave, a synthesised irregular model, or an imported eta record whose components are set
// (not NoWave, no model, a record without them)
bool kin_has_components(const hc_ctx* c);
// A synthesised irregular model (irregular without an imported eta record, or spectral): the ramp and Wheeler stretching apply to it.
// A record is used as given, with or without components: no ramp (kin_ramp is 1)
bool kin_synthesised(const hc_ctx* c);
// The ramp factor of the first-order quantities at time t (that of the spectral excitation, hc_kernels.hip): a synthesised model with
// ramp_duration > 0 rises as max(t, 0) / ramp_duration up to ramp_duration; 1 otherwise
double kin_ramp(const hc_ctx* c, double t);
// A path's own copy of the table, built at wave_serial `serial` for the regular phase `cached_phase`, is still the one in force for
// `phase`: no hc_set_wave_* call has come in since and, for a regular wave, the phase has the same bits
bool kin_table_current(const hc_ctx* c, unsigned long long serial, double cached_phase, double phase);

// The two direction columns [2][nf] (cos theta_i, then sin theta_i) of the directions in force (hc_set_wave_directions); empty when
// none are set.  A path that sums the directional sea appends them behind its own table's columns.
constexpr int kDirCols = 2;
std::vector<double> kin_dir_columns_host(const hc_ctx* c);

// k (x cos + y sin) of the directional instantiations / k x of the long-crested ones, whose expression stays the one it was
template <bool DIR>
__host__ __device__ __forceinline__ double kin_kx(double k, double x, double y, double dc, double ds) {
    if constexpr (DIR)
        return k * (x * dc + y * ds);
    else
        return k * x;
}

}  // namespace hc
