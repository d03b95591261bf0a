/* rkfd_emu_links.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The lane emulator of rkfd_emu.cpp (included whole: the same wavefront primitives) with one more entry point, rkfd_emu_links: the
 * device code of the task-space read-out (roki-fd_amd/csrc/readout/rkfd_links.h, what rkfdBatchUpdateLinks launches) on 64 host
 * threads, with the tables rkfd_capi_links.hip builds (rkfd_links_host_build) and - par_mass / par_com not NULL - the model-space
 * rows of a table of per-instance parameters, laid out as the C ABI lays them out.  tests/test_emu_links.py drives it.
 */
#include "rkfd_emu.cpp"
#include "readout/rkfd_links.h"
#include "readout/rkfd_links_host.h"

/* dis / vel [batch][ndof]; par_mass [batch][nlink] and par_com [batch][nlink*3] or both NULL; results as rkfdBatchGetLinks gives
 * them (pointers of quantities the flags do not select may be NULL) */
extern "C" int rkfd_emu_links(const rkfdModel *m, int batch, const double *dis, const double *vel, int flags,
                              const double *par_mass, const double *par_com, double *R, double *p, double *v, double *com, double *comvel)
{
  rkfdDevModelHost h;
  char err[256];
  if( rkfd_devmodel_build( m, 0, &h, err, sizeof(err) ) < 0 ) return -1;
  rkfdLinksHostTab ht;
  rkfd_links_host_build( m, &h, &ht );
  const size_t NLM = m->nlink;
  rkfdLinksTab t;
  t.nlink = h.dm.nlink; t.nlink_model = m->nlink; t.nchain = m->nchain; t.ndof = m->ndof; t.nround = h.dm.nround;
  t.linfo = h.dm.linfo; t.anc = h.dm.anc;
  t.dorg = ht.dorg.data(); t.dpre = ht.dpre.data(); t.mvel = ht.mvel.data();
  t.mdev = ht.mdev.data(); t.mframe = ht.mframe.data(); t.chain_off = ht.chain_off.data(); t.chain_idx = ht.chain_idx.data();
  t.mass = ht.masscom.data(); t.com = ht.masscom.data() + NLM; t.par_stride = 0;
  std::vector<double> rows;
  if( par_mass && par_com ){
    rows.resize( (size_t)batch*4*NLM + 1 );
    for( size_t i=0; i<(size_t)batch; i++ ){
      memcpy( &rows[i*4*NLM], par_mass + i*NLM, sizeof(double)*NLM );
      memcpy( &rows[i*4*NLM + NLM], par_com + i*3*NLM, sizeof(double)*3*NLM );
    }
    t.mass = rows.data(); t.com = rows.data() + NLM; t.par_stride = (int)( 4*NLM );
  }
  std::vector<double> lds( RKFD_LINKS_LDS_DOUBLES( t.nlink, t.nlink_model, t.nchain ) + 8 );
  for( int b=0; b<batch; b++ ){
    std::barrier<> bar0( 64 );
    g_bars[0] = &bar0;
    std::memset( lds.data(), 0xFF, sizeof(double)*lds.size() );      /* (poisoned, as in rkfd_emu_run: LDS is not cleared on the GPU) */
    std::vector<std::thread> th;
    for( int l=0; l<64; l++ )
      th.emplace_back( [&, l](){ t_tid = l; rkfd_links_instance( t, dis, vel, (size_t)b, LANE(), lds.data(), flags, R, p, v, com, comvel ); } );
    for( auto &x : th ) x.join();
  }
  rkfd_devmodel_free( &h );
  return 0;
}
