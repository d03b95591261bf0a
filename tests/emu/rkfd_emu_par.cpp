/* rkfd_emu_par.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The lane emulator of rkfd_emu.cpp (included whole: the same wavefront primitives, the same rkfd_emu_run) with one more entry
 * point, rkfd_emu_run_par: a launch with a table of per-instance physical parameters, as rkfdBatchSetParam leaves it - par[key] is
 * the model-space array [batch][width] of key RKFD_PAR_* (include/rkfd_hip.h), the rows are made by rkfd_devmodel_par_row, the
 * model's pointers are bound to the table by rkfd_devmodel_par_bind and every instance gets the row stride, exactly as
 * rkfd_capi.hip's launch does.  par = NULL: no table (rkfd_emu_run's launch).
 * Built once per RKFD_W (librkfd_emu_par.so, librkfd_emu_par_w2.so); tests/test_emu_params.py drives it.
 */
#include "rkfd_emu.cpp"

extern "C" int rkfd_emu_run_par(const rkfdModel *m, int max_rigid, rkfdDevState *st, int mode, int nsteps, const double *const *par)
{
  rkfdDevModelHost h;
  char err[256];
  if( rkfd_devmodel_build_w( m, max_rigid, 8/RKFD_W, &h, err, sizeof(err) ) < 0 ) return -1;
  if( h.ncand > 0 ) rkfd_ref_to_device( &h, st->cv_ref, (size_t)st->batch*h.ncand );
  rkfdDevModel dm = h.dm;
  const int stride = par ? (int)rkfd_devmodel_par_stride( &h ) : 0;
  std::vector<double> table( (size_t)stride*st->batch + 1 );
  if( par ){
    for( int i=0; i<st->batch; i++ ){
      const double *row_par[13];
      for( int k=0; k<13; k++ ){
        const int w = k >= 7 ? m->nci : m->nlink*( k == 1 ? 3 : ( k == 2 ? 9 : 1 ) );
        row_par[k] = par[k] + (size_t)i*w;
      }
      rkfd_devmodel_par_row( &h, row_par, &table[(size_t)i*stride] );
    }
    rkfd_devmodel_par_bind( &dm, table.data() );
  }
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
        if( dm.vol_np > 0 ) rkfd_instance<false, 2, false>( dm, *st, bi, base, mode, nsteps, &errflag, true, shared, nullptr, 0, stride );
        else if( dm.vert_rigid ) rkfd_instance<false, 1, false>( dm, *st, bi, base, mode, nsteps, &errflag, true, shared, nullptr, 0, stride );
        else if( dm.ma_packed ) rkfd_instance<false, 0, true>( dm, *st, bi, base, mode, nsteps, &errflag, true, shared, nullptr, 0, stride );
        else rkfd_instance<false, 0, false>( dm, *st, bi, base, mode, nsteps, &errflag, true, shared, nullptr, 0, stride ); } );
    }
    for( auto &t : th ) t.join();
  }
  if( h.ncand > 0 ) rkfd_ref_to_model( &h, st->cv_ref, (size_t)st->batch*h.ncand );
  rkfd_devmodel_free( &h );
  return errflag;
}
