// mom_mie_ab.hpp -- the Mie coefficient kernel of mom_mie.hip (k_mie_ab) on its own: a_n, b_n of a list of size parameters, left on
// the device.  mom_mie_coefficients(_dual) and the PCW route (mom_pcw.hip) both go through it.  The kernel and the host text around it
// (get_n_max, the start of the downward recurrence, sin x and cos x from the host library) live in mom_mie.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace mom_mie_ab {

// get_n_max (mie_helper_functions.jl:17)
int n_max_of(double x);

// What launch() needs besides the planes, in bytes: the D planes [n_max, ld] (two; Dual: four), x, sin x, cos x [ld] and the integers.
size_t workspace_bytes(int n_max, size_t ld, bool dual = false);

// a_n, b_n (unscaled, as mom_mie_coefficients writes them) of the nX size parameters x (host, positive) on stream st: four planes
// Re a, Im a, Re b, Im b, plane q at d_planes + q * plane_stride, each [>= n_max rows, ld] with x fastest (ld >= nX); the caller
// has zeroed them, and the kernel leaves the rows above each x's own n_max,i alone.  dual: the Dual form, four more planes da / dm,
// db / dm (plane 4 .. 7).  h_nmax [nX], when given, receives n_max,i; *d_nmax the device copy of it (inside d_ws, [ld], zeros beyond
// nX).  ev0 / ev1, when given, are recorded around the kernel.  The uploads are complete when the call returns.
// MOM_EINVAL (text through mom_set_global_error, starting with fn): an n_max,i above n_max.
int launch(const char *fn, hipStream_t st, int nX, size_t ld, const double *x, double n_r, double n_i, int n_max, size_t plane_stride,
           double *d_planes, char *d_ws, int *h_nmax, const int **d_nmax, hipEvent_t ev0, hipEvent_t ev1, bool dual = false);

}  // namespace mom_mie_ab
