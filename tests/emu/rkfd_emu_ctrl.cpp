/* rkfd_emu_ctrl.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The lane emulator of rkfd_emu.cpp (included whole: the same wavefront primitives, the same rkfd_emu_run) with one more entry
 * point, rkfd_emu_run_ctrl: nsteps x rkFDUpdate under a control schedule - the launch rkfdBatchUpdateControlled makes for one
 * round of steps, with `ctrl` pointing at the round's first step and `ctrl_stride` the doubles of one instance's whole schedule.
 * Built once per RKFD_W (librkfd_emu_ctrl.so, librkfd_emu_ctrl_w2.so); tests/test_emu_control.py drives it.
 */
#include "rkfd_emu.cpp"

extern "C" int rkfd_emu_run_ctrl(const rkfdModel *m, int max_rigid, rkfdDevState *st, int nsteps, const double *ctrl, int ctrl_stride)
{
  rkfdDevModelHost h;
  char err[256];
  if( rkfd_devmodel_build_w( m, max_rigid, 8/RKFD_W, &h, err, sizeof(err) ) < 0 ) return -1;
  if( h.ncand > 0 ) rkfd_ref_to_device( &h, st->cv_ref, (size_t)st->batch*h.ncand );
  std::vector<char> lds( RKFD_W*h.lds_bytes + h.dm.lds_shared + 64 );
  int errflag = 0;
  for( int b=0; b<st->batch; b+=RKFD_W ){
    std::barrier<> bar0( EMU_WL ), bar1( EMU_WL );
    g_bars[0] = &bar0; if( RKFD_W > 1 ) g_bars[RKFD_W-1] = &bar1;
    int nrun = 0;
    for( int l=0; l<64; l++ ) nrun += b + l/EMU_WL < st->batch;
    std::barrier<> wbar( nrun );
    g_wavebar = &wbar;
    std::memset( lds.data(), 0xFF, lds.size() );      /* (poisoned, as in rkfd_emu_run) */
    std::vector<std::thread> th;
    for( int l=0; l<64; l++ ){
      if( b + l/EMU_WL >= st->batch ) continue;
      th.emplace_back( [&, l](){ t_tid = l;
        const int bi = b + l/EMU_WL;
        char *base = lds.data() + ( l/EMU_WL )*h.lds_bytes;
        char *shared = lds.data() + RKFD_W*h.lds_bytes;
        if( h.dm.vol_np > 0 ) rkfd_instance<false, 2, false>( h.dm, *st, bi, base, 0, nsteps, &errflag, true, shared, ctrl, ctrl_stride );
        else if( h.dm.vert_rigid ) rkfd_instance<false, 1, false>( h.dm, *st, bi, base, 0, nsteps, &errflag, true, shared, ctrl, ctrl_stride );
        else if( h.dm.ma_packed ) rkfd_instance<false, 0, true>( h.dm, *st, bi, base, 0, nsteps, &errflag, true, shared, ctrl, ctrl_stride );
        else rkfd_instance<false, 0, false>( h.dm, *st, bi, base, 0, nsteps, &errflag, true, shared, ctrl, ctrl_stride ); } );
    }
    for( auto &t : th ) t.join();
  }
  if( h.ncand > 0 ) rkfd_ref_to_model( &h, st->cv_ref, (size_t)st->batch*h.ncand );
  rkfd_devmodel_free( &h );
  return errflag;
}
