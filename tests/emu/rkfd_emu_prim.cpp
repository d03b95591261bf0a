/* rkfd_emu_prim.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The lane emulator of rkfd_emu.cpp (included whole: the same build of the device headers) with four more entry points: plain loops
 * over the rotation primitives of roki-fd_amd/csrc/device/rkfd_dev_base.h - d_sincos, d_atan2_ypos, d_from_aa, d_to_aa - one call per
 * element, no lanes involved.  tests/test_rot_primitives.py compares them with long double.
 */
#include "rkfd_emu.cpp"

/* sn[i], cs[i] = d_sincos( x[i] ) */
extern "C" void rkfd_emu_prim_sincos(int n, const double *x, double *sn, double *cs)
{
  for( int i=0; i<n; i++ ) d_sincos( x[i], sn+i, cs+i );
}

/* r[i] = d_atan2_ypos( y[i], x[i] ), y[i] >= 0 */
extern "C" void rkfd_emu_prim_atan2_ypos(int n, const double *y, const double *x, double *r)
{
  for( int i=0; i<n; i++ ) r[i] = d_atan2_ypos( y[i], x[i] );
}

/* m[9 i .. 9 i + 8] (row-major) = d_from_aa( aa[3 i .. 3 i + 2] ) */
extern "C" void rkfd_emu_prim_from_aa(int n, const double *aa, double *m)
{
  for( int i=0; i<n; i++ ) d_from_aa( aa + 3*i, m + 9*i );
}

/* aa[3 i .. 3 i + 2] = d_to_aa( m[9 i .. 9 i + 8] ) */
extern "C" void rkfd_emu_prim_to_aa(int n, const double *m, double *aa)
{
  for( int i=0; i<n; i++ ) d_to_aa( m + 9*i, aa + 3*i );
}
