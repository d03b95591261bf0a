/* rkfd_emu_jac.cpp - DEVELOPMENT / TEST HARNESS ONLY.
 *
 * The lane emulator of rkfd_emu.cpp (included whole: the same wavefront primitives) with one more entry point, rkfd_emu_jac: the
 * device code of the task-space Jacobians (roki-fd_amd/csrc/readout/rkfd_jac.h, what rkfdBatchUpdateJacobians launches) on 64 host
 * threads, with the tables rkfd_capi_jac.hip builds (rkfd_jac_host_build), the sites checked as rkfdBatchSetJacobianSites checks
 * them and - par_mass / par_com not NULL - the model-space rows of a table of per-instance parameters, laid out as the C ABI lays
 * them out.  tests/test_emu_jac.py drives it.
 */
#include "rkfd_emu.cpp"
#include "readout/rkfd_jac.h"
#include "readout/rkfd_jac_host.h"

/* dis [batch][ndof]; site_link [nsite], site_point [nsite][3] or NULL; par_mass [batch][nlink] and par_com [batch][nlink*3] or both
 * NULL; results as rkfdBatchGetJacobians gives them (the pointer of a quantity the flags do not select may be NULL).  -2: the
 * sites were refused. */
extern "C" int rkfd_emu_jac(const rkfdModel *m, int batch, const double *dis, int flags, int nsite, const int *site_link, const double *site_point,
                            const double *par_mass, const double *par_com, double *J, double *Jcom)
{
  char err[256];
  if( m->ndof > RKFD_WAVE ) return -1;
  if( rkfd_jac_check_sites( m->nlink, nsite, site_link, site_point, err, sizeof(err) ) < 0 ) return -2;
  rkfdJacHostTab ht;
  rkfd_jac_host_build( m, &ht );
  const size_t NLM = m->nlink;
  std::vector<double> pts( (size_t)3*nsite + 1, 0.0 );
  if( site_point ) memcpy( pts.data(), site_point, sizeof(double)*3*nsite );
  rkfdJacTab t;
  t.nlink = m->nlink; t.nchain = m->nchain; t.ndof = m->ndof; t.nsite = nsite;
  t.parent = m->parent; t.jtype = m->jtype; t.dofoff = m->dofoff; t.org = m->org;
  t.cown = ht.cown.data(); t.chain_off = ht.chain_off.data(); t.chain_idx = ht.chain_idx.data();
  t.site_link = site_link; t.site_point = pts.data();
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
  std::vector<double> lds( RKFD_JAC_LDS_DOUBLES( t.nlink, t.ndof ) + 8 );
  for( int b=0; b<batch; b++ ){
    std::barrier<> bar0( 64 );
    g_bars[0] = &bar0;
    std::memset( lds.data(), 0xFF, sizeof(double)*lds.size() );      /* (poisoned, as in rkfd_emu_run: LDS is not cleared on the GPU) */
    std::vector<std::thread> th;
    for( int l=0; l<64; l++ )
      th.emplace_back( [&, l](){ t_tid = l; rkfd_jac_instance( t, dis, (size_t)b, LANE(), lds.data(), flags, J, Jcom ); } );
    for( auto &x : th ) x.join();
  }
  return 0;
}
