/* rkfd_emu_cf.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The lane emulator of rkfd_emu.cpp (included whole: the same wavefront primitives) with one more entry point, rkfd_emu_cf: the
 * device code of the contact read-out (roki-fd_amd/csrc/readout/rkfd_cf.h, what rkfdBatchUpdateContactForces launches) on 64 host
 * threads, with the tables rkfd_capi_cf.hip builds (rkfd_cf_host_build) or - own not NULL - with candidate tables of the caller's:
 * synthetic candidates on any tree, without a contact solver.  tests/test_emu_cf.py drives it.
 */
#include "rkfd_emu.cpp"
#include "readout/rkfd_cf.h"
#include "readout/rkfd_cf_host.h"

/* dis [batch][ndof], active [batch][nc], f [batch][nc*3] with nc = the model's ncand, or ncand when own / oth [ncand] and vert
 * [ncand*3] are given; results as rkfdBatchGetContactForces gives them (the pointer of a quantity the flags do not select may be
 * NULL).  -1: more than 64 coordinates; -2: a candidate names a link out of range; otherwise the instances per workgroup
 * rkfd_capi_cf.hip would choose (0: one instance does not fit the LDS). */
extern "C" int rkfd_emu_cf(const rkfdModel *m, int batch, const double *dis, const int *active, const double *f, int flags,
                           int ncand, const int *own, const int *oth, const double *vert,
                           double *point, double *wrench, int *count, double *genf)
{
  if( m->ndof > RKFD_WAVE ) return -1;
  rkfdCfHostTab ht;
  if( rkfd_cf_host_build( m, ncand, own, oth, vert, &ht, NULL, 0 ) < 0 ) return -2;
  rkfdCfTab t;
  std::memset( &t, 0, sizeof(t) );
  t.j.nlink = m->nlink; t.j.nchain = m->nchain; t.j.ndof = m->ndof;
  t.j.parent = m->parent; t.j.jtype = m->jtype; t.j.dofoff = m->dofoff; t.j.org = m->org; t.j.cown = ht.cown.data();
  t.ncand = ht.ncand;
  t.c_own = ht.c_own.data(); t.c_oth = ht.c_oth.data(); t.c_vert = ht.c_vert.data(); t.l_off = ht.l_off.data(); t.l_ent = ht.l_ent.data();
  const size_t nlds = RKFD_CF_LDS_DOUBLES( m->nlink, m->ndof );
  std::vector<double> lds( nlds + 8 );
  for( int b=0; b<batch; b++ ){
    std::barrier<> bar0( 64 );
    g_bars[0] = &bar0;
    std::memset( lds.data(), 0xFF, sizeof(double)*lds.size() );      /* (poisoned, as in rkfd_emu_run: LDS is not cleared on the GPU) */
    std::vector<std::thread> th;
    for( int l=0; l<64; l++ )
      th.emplace_back( [&, l](){ t_tid = l; rkfd_cf_instance( t, dis, active, f, (size_t)b, LANE(), lds.data(), flags, point, wrench, count, genf ); } );
    for( auto &x : th ) x.join();
  }
  return rkfd_cf_host_waves( sizeof(double)*nlds );
}
