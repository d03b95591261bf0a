/* rkfd_emu_reset.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The device code of the per-instance reset (roki-fd_amd/csrc/reset/rkfd_reset.h, what rkfdBatchReset launches) on the host, over
 * the grid rkfd_capi_reset.hip launches: workgroups of RKFD_RESET_WAVES wavefronts of 64 lanes over the instances [first, end).
 * The lanes of a wavefront exchange nothing and there is no barrier, so they run one after the other.  The state, the bank and
 * the snapshot are the caller's arrays (tests/emu/emu.py: EmuBatch's, and numpy arrays laid out the same way).
 * tests/test_emu_reset.py drives it.
 */
#define RKFD_EMU
#include "reset/rkfd_reset.h"

/* snap: NULL when no snapshot was taken; returns the error flag the launch left (0, or RKFD_RESET_STATUS) */
extern "C" int rkfd_emu_reset(const rkfdDevState *st, const rkfdDevState *bank, int nslots, const rkfdDevState *snap, const int *slots,
                              int first, int end, int ND, int NL, int NC)
{
  rkfdDevState none = {};
  int errflag = 0;
  const unsigned blocks = (unsigned)( ( end - first + RKFD_RESET_WAVES - 1 )/RKFD_RESET_WAVES );
  for( unsigned blk=0; blk<blocks; blk++ )
    for( int wave=0; wave<RKFD_RESET_WAVES; wave++ )
      for( int lane=0; lane<RKFD_WAVE; lane++ )
        rkfd_reset_wavefront( *st, bank ? *bank : none, nslots, snap ? *snap : none, snap ? 1 : 0, slots, first, end, blk, wave, lane, ND, NL, NC, &errflag );
  return errflag;
}
