/* rkfd_reset.h - the per-instance reset (rkfdBatchReset): one instance's complete state copied from a row of a bank of start
 * states, or from the instance's own row of the whole-batch snapshot, while its neighbours run on.  One instance per 64-lane
 * wavefront; compiles for gfx950 (rkfd_capi_reset.hip) and under the lane emulator (tests/emu/rkfd_emu_reset.cpp).  It is no part
 * of the step kernels: it lives outside csrc/device/, so that the step kernels, their ahead-of-time code objects and their
 * resource reports do not depend on it.
 *
 * The bank is an rkfdDevState of `nslots` instances, the snapshot one of `batch` instances: one copy routine serves both, with
 * source row = slot or source row = instance.  A row is what rkfd_restore_kernel copies: dis, vel, acc, piv_type, piv_prev, brk,
 * cv_active, cv_type, cv_ref, cv_f.  Motor input, parameters and the contact statistics are not state here. */
#ifndef RKFD_RESET_H
#define RKFD_RESET_H

#include <stddef.h>
#include "rkfd_model.h"
#include "rkfd_devmodel.h"

#define RKFD_RESET_KEEP_V     ( -1 )     /* RKFD_RESET_KEEP, RKFD_RESET_SNAPSHOT of include/rkfd_hip.h */
#define RKFD_RESET_SNAPSHOT_V ( -2 )
#define RKFD_RESET_STATUS     5          /* rkfdBatchStatus: a slot value that names no row */
#define RKFD_RESET_WAVES      4          /* instances (wavefronts) of one workgroup */

#ifdef RKFD_EMU
#  define RKFD_RESET_DEV static inline
#  define RKFD_RESET_UNIFORM(x) (x)      /* (every thread of the emulated wavefront has read the same value) */
#else
#  define RKFD_RESET_DEV __device__ __forceinline__
#  define RKFD_RESET_UNIFORM(x) __builtin_amdgcn_readfirstlane( x )
#endif

/* row `s` of src into row `d` of dst: consecutive lanes move consecutive elements */
RKFD_RESET_DEV void rkfd_reset_copy_row(const rkfdDevState &dst, size_t d, const rkfdDevState &src, size_t s, int lane, int ND, int NL, int NC)
{
  for( int j=lane; j<ND; j+=RKFD_WAVE ){
    dst.dis[d*ND+j] = src.dis[s*ND+j]; dst.vel[d*ND+j] = src.vel[s*ND+j]; dst.acc[d*ND+j] = src.acc[s*ND+j];
  }
  for( int j=lane; j<NL; j+=RKFD_WAVE ){
    dst.piv_type[d*NL+j] = src.piv_type[s*NL+j]; dst.piv_prev[d*NL+j] = src.piv_prev[s*NL+j];
    dst.brk[d*NL+j] = src.brk[s*NL+j];
  }
  for( int j=lane; j<NC; j+=RKFD_WAVE ){
    dst.cv_active[d*NC+j] = src.cv_active[s*NC+j]; dst.cv_type[d*NC+j] = src.cv_type[s*NC+j];
  }
  for( int j=lane; j<3*NC; j+=RKFD_WAVE ){
    dst.cv_ref[d*3*NC+j] = src.cv_ref[s*3*NC+j]; dst.cv_f[d*3*NC+j] = src.cv_f[s*3*NC+j];
  }
}

/* instance b (the caller has checked that it is one of the batch) does what slots[b] says.  The value is read once and made
 * uniform over the wavefront, so the KEEP exit is a scalar branch taken before any other memory access.  bank: nslots rows (no
 * pointer of it is touched when nslots = 0); snap: the whole-batch snapshot, has_snap = 0 when none was taken.  A value that names
 * no row leaves the instance as it is and sets *errflag. */
RKFD_RESET_DEV void rkfd_reset_instance(const rkfdDevState &st, const rkfdDevState &bank, int nslots, const rkfdDevState &snap, int has_snap,
                                        const int *slots, size_t b, int lane, int ND, int NL, int NC, int *errflag)
{
  const int s = RKFD_RESET_UNIFORM( slots[b] );
  if( s == RKFD_RESET_KEEP_V ) return;
  if( s >= 0 && s < nslots ) rkfd_reset_copy_row( st, b, bank, (size_t)s, lane, ND, NL, NC );
  else if( s == RKFD_RESET_SNAPSHOT_V && has_snap ) rkfd_reset_copy_row( st, b, snap, b, lane, ND, NL, NC );
  else if( lane == 0 ) *errflag = RKFD_RESET_STATUS;
}

/* wavefront `wave` of workgroup `block` of a launch over the instances [first, end): its instance, if it has one (the last workgroup
 * may be partial) */
RKFD_RESET_DEV void rkfd_reset_wavefront(const rkfdDevState &st, const rkfdDevState &bank, int nslots, const rkfdDevState &snap, int has_snap,
                                         const int *slots, int first, int end, unsigned block, int wave, int lane, int ND, int NL, int NC, int *errflag)
{
  const size_t b = (size_t)first + (size_t)block*RKFD_RESET_WAVES + (size_t)wave;
  if( b >= (size_t)end ) return;
  rkfd_reset_instance( st, bank, nslots, snap, has_snap, slots, b, lane, ND, NL, NC, errflag );
}

#endif /* RKFD_RESET_H */
