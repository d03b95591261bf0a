/* rkfd_emu_dyn.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The lane emulator of rkfd_emu.cpp (included whole: the same wavefront primitives) with one more entry point, rkfd_emu_dyn: the
 * device code of the joint-space dynamics (roki-fd_amd/csrc/readout/rkfd_dyn.h, what rkfdBatchUpdateDynamics launches) on 64 host
 * threads, with the tables rkfd_capi_dyn.hip builds (rkfd_dyn_host_build) and - par_mass / par_com / par_inertia not NULL - the
 * model-space rows of a table of per-instance parameters, laid out as the C ABI lays them out.  tests/test_emu_dyn.py drives it.
 */
#include "rkfd_emu.cpp"
#include "readout/rkfd_dyn.h"
#include "readout/rkfd_dyn_host.h"

/* dis, vel [batch][ndof]; par_mass [batch][nlink], par_com [batch][nlink*3] and par_inertia [batch][nlink*9] or all NULL; results as
 * rkfdBatchGetDynamics gives them (the pointer of a quantity the flags do not select may be NULL).  -1: more than 64 coordinates;
 * otherwise the instances per workgroup rkfd_capi_dyn.hip would choose (0: one instance does not fit the LDS). */
extern "C" int rkfd_emu_dyn(const rkfdModel *m, int batch, const double *dis, const double *vel, int flags,
                            const double *par_mass, const double *par_com, const double *par_inertia, double *M, double *h, double *g)
{
  if( m->ndof > RKFD_WAVE ) return -1;
  rkfdDynHostTab ht;
  rkfd_dyn_host_build( m, &ht );
  const size_t NLM = m->nlink;
  rkfdDynTab t;
  t.nlink = m->nlink; t.ndof = m->ndof; t.nlevel = ht.nlevel;
  t.parent = m->parent; t.jtype = m->jtype; t.dofoff = m->dofoff; t.org = m->org;
  t.cown = ht.cown.data(); t.lev_off = ht.lev_off.data(); t.lev_idx = ht.lev_idx.data();
  t.child_off = ht.child_off.data(); t.child_idx = ht.child_idx.data(); t.amask = ht.amask.data(); t.rotor = ht.rotor.data();
  t.mass = ht.mci.data(); t.com = ht.mci.data() + NLM; t.inertia = ht.mci.data() + 4*NLM; t.par_stride = 0;
  std::vector<double> rows;
  if( par_mass && par_com && par_inertia ){
    rkfd_dyn_host_rows( m->nlink, (size_t)batch, par_mass, par_com, par_inertia, &rows );
    t.mass = rows.data(); t.com = rows.data() + NLM; t.inertia = rows.data() + 4*NLM; t.par_stride = (int)( 13*NLM );
  }
  const size_t nlds = RKFD_DYN_LDS_DOUBLES( t.nlink, t.ndof );
  std::vector<double> lds( nlds + 8 );
  for( int b=0; b<batch; b++ ){
    std::barrier<> bar0( 64 );
    g_bars[0] = &bar0;
    std::memset( lds.data(), 0xFF, sizeof(double)*lds.size() );      /* (poisoned, as in rkfd_emu_run: LDS is not cleared on the GPU) */
    std::vector<std::thread> th;
    for( int l=0; l<64; l++ )
      th.emplace_back( [&, l](){ t_tid = l; rkfd_dyn_instance( t, dis, vel, (size_t)b, LANE(), lds.data(), flags, M, h, g ); } );
    for( auto &x : th ) x.join();
  }
  return rkfd_dyn_host_waves( sizeof(double)*nlds );
}
