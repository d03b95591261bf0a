/* rkfd_capi_jac.hip - the task-space Jacobians behind rkfdBatchUpdateJacobians (include/rkfd_hip.h): one kernel that computes the
 * site Jacobians and the centre-of-mass Jacobian of every chain from the live joint coordinates (readout/rkfd_jac.h), its tables, its
 * sites and its result buffers.  A translation unit of its own, as rkfd_capi_links.hip is: the step kernels of rkfd_capi.hip and
 * the read-out's kernel stay what they are to the instruction; this kernel's resource report goes to kernel_resources_jac.txt. */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
/* (rkfd_dev_base.h's __constant__ table needs a name of its own in every translation unit: see rkfd_capi_links.hip) */
#define rkfd_kc rkfd_kc_jac
#include "readout/rkfd_jac.h"
#include "readout/rkfd_jac_host.h"

/* one instance per wavefront, RKFD_LINKS_WAVES of them per workgroup; every wavefront works in its own piece of the workgroup's
 * LDS and returns on its own when its instance is beyond the batch (there is no workgroup barrier) */
extern "C" __global__ void __launch_bounds__(RKFD_WAVE*RKFD_LINKS_WAVES)
rkfd_jac_kernel(rkfdJacTab t, const double *dis, int batch, int flags, int lds_doubles, double *oJ, double *oJcom)
{
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = LANE();
  const int wave = tid >> 6, lane = tid & ( RKFD_WAVE-1 );
  const size_t b = (size_t)blockIdx.x*RKFD_LINKS_WAVES + wave;
  if( b >= (size_t)batch ) return;
  rkfd_jac_instance( t, dis, b, lane, (double *)lds + (size_t)wave*lds_doubles, flags, oJ, oJcom );
}

#define LFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); return -1; }while(0)
#define LHIP(call) do{ hipError_t e_ = (call); if( e_ != hipSuccess ) LFAIL( "%s failed: %s", #call, hipGetErrorString( e_ ) ); }while(0)

struct rkfdJac {
  int batch, nlink, nchain, ndof, nsite;
  rkfdJacTab tab;
  void *dblob;            /* parent | jtype | dofoff | cown | chain_off | chain_idx | org | masscom, on the device */
  int *d_site_link;       /* [RKFD_JAC_MAX_SITES] */
  double *d_site_point;   /* [RKFD_JAC_MAX_SITES*3] */
  double *d_shared;       /* the model's masses and centres of mass inside dblob */
  double *d_par;          /* [batch][4 nlink]: the instances' own (allocated by the first launch of a batch with a table) */
  int par_gen;            /* generation of the table d_par holds (-1: none) */
  int lds_doubles;
  double *out[2];         /* J, Jcom */
  int flags;              /* of the last launch, less RKFD_JAC_F_SITES once the sites were replaced */
  hipEvent_t done;
};

extern "C" rkfdJac *rkfd_jac_create(const rkfdModel *m, int batch, char *err, int errlen)
{
#define CFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); rkfd_jac_destroy( j ); return NULL; }while(0)
  rkfdJac *j = (rkfdJac *)calloc( 1, sizeof(rkfdJac) );
  if( !j ){ if( err ) snprintf( err, errlen, "out of memory" ); return NULL; }
  const int NLM = m->nlink, NCH = m->nchain, ND = m->ndof;
  j->batch = batch; j->nlink = NLM; j->nchain = NCH; j->ndof = ND; j->par_gen = -1;
  if( ND > RKFD_WAVE ) CFAIL( "rkfdBatchUpdateJacobians: %d joint coordinates exceed the %d lanes of a wavefront", ND, RKFD_WAVE );
  j->lds_doubles = RKFD_JAC_LDS_DOUBLES( NLM, ND );
  const size_t lds = sizeof(double)*(size_t)j->lds_doubles*RKFD_LINKS_WAVES;
  if( lds > 160*1024 ) CFAIL( "rkfdBatchUpdateJacobians: a world of %d links and %d joint coordinates needs %zu bytes of LDS per workgroup (> 160 KiB)", NLM, ND, lds );
  if( lds > 64*1024 && hipFuncSetAttribute( (const void *)rkfd_jac_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateJacobians: hipFuncSetAttribute(LDS=%zu) failed", lds );
  rkfdJacHostTab ht;
  rkfd_jac_host_build( m, &ht );
  const size_t nl1 = NLM > 0 ? NLM : 1;
  const size_t ni = 3*nl1 + ht.cown.size() + ht.chain_off.size() + ht.chain_idx.size(), ni2 = ( ni + 1 ) & ~(size_t)1;      /* (the doubles start 8-byte aligned) */
  const size_t nd = 12*nl1 + ht.masscom.size();
  const size_t bytes = sizeof(int)*ni2 + sizeof(double)*nd;
  std::vector<char> blob( bytes, 0 );
  int *ip = (int *)blob.data();
  double *dp = (double *)( blob.data() + sizeof(int)*ni2 );
  const size_t o_par = 0, o_jt = nl1, o_off = 2*nl1, o_own = 3*nl1, o_co = o_own + ht.cown.size(), o_ci = o_co + ht.chain_off.size();
  memcpy( ip + o_par, m->parent, sizeof(int)*NLM ); memcpy( ip + o_jt, m->jtype, sizeof(int)*NLM ); memcpy( ip + o_off, m->dofoff, sizeof(int)*NLM );
  memcpy( ip + o_own, ht.cown.data(), sizeof(int)*ht.cown.size() );
  memcpy( ip + o_co, ht.chain_off.data(), sizeof(int)*ht.chain_off.size() );
  memcpy( ip + o_ci, ht.chain_idx.data(), sizeof(int)*ht.chain_idx.size() );
  memcpy( dp, m->org, sizeof(double)*12*NLM );
  memcpy( dp + 12*nl1, ht.masscom.data(), sizeof(double)*ht.masscom.size() );
  if( hipMalloc( &j->dblob, bytes ) != hipSuccess || hipMemcpy( j->dblob, blob.data(), bytes, hipMemcpyHostToDevice ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateJacobians: cannot copy the model tables to the device" );
  if( hipMalloc( (void **)&j->d_site_link, sizeof(int)*RKFD_JAC_MAX_SITES ) != hipSuccess ||
      hipMalloc( (void **)&j->d_site_point, sizeof(double)*3*RKFD_JAC_MAX_SITES ) != hipSuccess ||
      hipMemset( j->d_site_link, 0, sizeof(int)*RKFD_JAC_MAX_SITES ) != hipSuccess ||
      hipMemset( j->d_site_point, 0, sizeof(double)*3*RKFD_JAC_MAX_SITES ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateJacobians: cannot allocate the site tables on the device" );
  if( hipEventCreateWithFlags( &j->done, hipEventDisableTiming ) != hipSuccess ) CFAIL( "rkfdBatchUpdateJacobians: hipEventCreate failed" );
  const int *dip = (const int *)j->dblob;
  const double *ddp = (const double *)( (const char *)j->dblob + sizeof(int)*ni2 );
  rkfdJacTab &t = j->tab;
  t.nlink = NLM; t.nchain = NCH; t.ndof = ND; t.nsite = 0;
  t.parent = dip + o_par; t.jtype = dip + o_jt; t.dofoff = dip + o_off; t.cown = dip + o_own; t.chain_off = dip + o_co; t.chain_idx = dip + o_ci;
  t.org = ddp;
  t.site_link = j->d_site_link; t.site_point = j->d_site_point;
  j->d_shared = (double *)ddp + 12*nl1;
  return j;
#undef CFAIL
}

extern "C" void rkfd_jac_destroy(rkfdJac *j)
{
  if( !j ) return;
  if( j->done ){ (void)hipEventSynchronize( j->done ); (void)hipEventDestroy( j->done ); }
  for( int k=0; k<2; k++ ) (void)hipFree( j->out[k] );
  (void)hipFree( j->d_par ); (void)hipFree( j->d_site_link ); (void)hipFree( j->d_site_point ); (void)hipFree( j->dblob );
  free( j );
}

extern "C" int rkfd_jac_nsite(const rkfdJac *j){ return j ? j->nsite : 0; }

extern "C" int rkfd_jac_set_sites(rkfdJac *j, int nsite, const int *link, const double *point, char *err, int errlen)
{
  if( rkfd_jac_check_sites( j->nlink, nsite, link, point, err, errlen ) < 0 ) return -1;
  /* (an earlier launch may still be reading the old sites and writing the old buffer) */
  LHIP( hipEventSynchronize( j->done ) );
  if( nsite > 0 ){
    std::vector<double> pt( (size_t)3*nsite, 0.0 );
    if( point ) memcpy( pt.data(), point, sizeof(double)*3*nsite );
    LHIP( hipMemcpy( j->d_site_link, link, sizeof(int)*nsite, hipMemcpyHostToDevice ) );
    LHIP( hipMemcpy( j->d_site_point, pt.data(), sizeof(double)*3*nsite, hipMemcpyHostToDevice ) );
  }
  if( nsite != j->nsite ){
    /* the buffer of another width goes; the next launch that needs one allocates it */
    (void)hipFree( j->out[0] ); j->out[0] = NULL;
  }
  j->nsite = nsite; j->tab.nsite = nsite;
  j->flags &= ~RKFD_JAC_F_SITES;      /* what the buffer holds, if anything, is not of these sites */
  return 0;
}

extern "C" int rkfd_jac_launch(rkfdJac *j, const double *dis, int flags, const double *par_mass, const double *par_com, int par_gen,
                               void *stream, char *err, int errlen)
{
  const size_t B = j->batch, NLM = j->nlink, NCH = j->nchain, ND = j->ndof;
  const hipStream_t s = (hipStream_t)stream;
  /* the buffers the selected quantities go to: allocated once (J: once per number of sites), stable afterwards */
  const size_t width[2] = { (size_t)j->nsite*6*ND, NCH*3*ND };
  const int need[2] = { flags & RKFD_JAC_F_SITES, flags & RKFD_JAC_F_COM };
  for( int k=0; k<2; k++ )
    if( need[k] && !j->out[k] ){
      const size_t n = B*width[k];
      /* (not cleared: the kernel writes every element of a selected array for every instance) */
      LHIP( hipMalloc( (void **)&j->out[k], sizeof(double)*( n ? n : 1 ) ) );
    }
  rkfdJacTab t = j->tab;
  t.mass = j->d_shared; t.com = j->d_shared + NLM; t.par_stride = 0;
  if( ( flags & RKFD_JAC_F_COM ) && par_mass && par_com ){
    if( par_gen != j->par_gen ){
      /* (rare: once per rkfdBatchSetParam.  An earlier launch may still be reading the old rows) */
      LHIP( hipEventSynchronize( j->done ) );
      if( !j->d_par ) LHIP( hipMalloc( (void **)&j->d_par, sizeof(double)*( B*4*NLM + 1 ) ) );
      std::vector<double> rows( B*4*NLM + 1 );
      for( size_t i=0; i<B; i++ ){
        memcpy( &rows[i*4*NLM], par_mass + i*NLM, sizeof(double)*NLM );
        memcpy( &rows[i*4*NLM + NLM], par_com + i*3*NLM, sizeof(double)*3*NLM );
      }
      LHIP( hipMemcpy( j->d_par, rows.data(), sizeof(double)*B*4*NLM, hipMemcpyHostToDevice ) );
      j->par_gen = par_gen;
    }
    t.mass = j->d_par; t.com = j->d_par + NLM; t.par_stride = (int)( 4*NLM );
  }
  const unsigned blocks = (unsigned)( ( B + RKFD_LINKS_WAVES - 1 )/RKFD_LINKS_WAVES );
  hipLaunchKernelGGL( rkfd_jac_kernel, dim3( blocks ), dim3( RKFD_WAVE*RKFD_LINKS_WAVES ), sizeof(double)*(size_t)j->lds_doubles*RKFD_LINKS_WAVES, s,
                      t, dis, j->batch, flags, j->lds_doubles, j->out[0], j->out[1] );
  LHIP( hipGetLastError() );
  LHIP( hipEventRecord( j->done, s ) );
  j->flags = flags;
  return 0;
}

extern "C" int rkfd_jac_flags(const rkfdJac *j){ return j ? j->flags : 0; }

extern "C" int rkfd_jac_get(rkfdJac *j, double *J, double *Jcom, char *err, int errlen)
{
  const size_t B = j->batch, NCH = j->nchain, ND = j->ndof;
  double *dst[2] = { J, Jcom };
  const size_t width[2] = { (size_t)j->nsite*6*ND, NCH*3*ND };
  LHIP( hipEventSynchronize( j->done ) );
  for( int k=0; k<2; k++ )
    if( dst[k] && B*width[k] ) LHIP( hipMemcpy( dst[k], j->out[k], sizeof(double)*B*width[k], hipMemcpyDeviceToHost ) );
  return 0;
}

extern "C" const double *rkfd_jac_dev(const rkfdJac *j, int which){ return ( j && which >= 0 && which < 2 ) ? j->out[which] : NULL; }
