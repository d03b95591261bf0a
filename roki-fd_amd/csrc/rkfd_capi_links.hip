/* rkfd_capi_links.hip - the task-space read-out behind rkfdBatchUpdateLinks (include/rkfd_hip.h): one kernel that computes the
 * poses and velocities of every model link and the centre of mass of every chain from the live joint state (readout/rkfd_links.h),
 * its tables and its result buffers.  A translation unit of its own, as rkfd_capi_par.hip is: the step kernels of rkfd_capi.hip
 * stay what they are to the instruction; this kernel's resource report goes to kernel_resources_links.txt. */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
/* rkfd_dev_base.h defines the __constant__ table rkfd_kc of d_sincos, which has a host-side symbol: every translation unit that
 * includes the header needs a name of its own for it.  rkfd_capi_par.hip does the same (rkfd_kc_par); the header is part of the
 * step kernels' hashed sources and is left alone.  Nothing in this file names rkfd_kc itself. */
#define rkfd_kc rkfd_kc_links
#include "readout/rkfd_links.h"
#include "readout/rkfd_links_host.h"

/* one instance per wavefront, RKFD_LINKS_WAVES of them per workgroup; every wavefront works in its own piece of the workgroup's
 * LDS and returns on its own when its instance is beyond the batch (there is no workgroup barrier).  The kernel is bound by its
 * loads and stores (2 ndof doubles in, 18 nlink_model doubles out per instance). */
extern "C" __global__ void __launch_bounds__(RKFD_WAVE*RKFD_LINKS_WAVES)
rkfd_links_kernel(rkfdLinksTab t, const double *dis, const double *vel, int batch, int flags, int lds_doubles,
                  double *oR, double *op, double *ov, double *ocom, double *ocomvel)
{
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = LANE();
  const int wave = tid >> 6, lane = tid & ( RKFD_WAVE-1 );
  const size_t b = (size_t)blockIdx.x*RKFD_LINKS_WAVES + wave;
  if( b >= (size_t)batch ) return;
  rkfd_links_instance( t, dis, vel, b, lane, (double *)lds + (size_t)wave*lds_doubles, flags, oR, op, ov, ocom, ocomvel );
}

#define LFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); return -1; }while(0)
#define LHIP(call) do{ hipError_t e_ = (call); if( e_ != hipSuccess ) LFAIL( "%s failed: %s", #call, hipGetErrorString( e_ ) ); }while(0)

struct rkfdLinks {
  int batch, nlink_model, nchain;
  rkfdLinksTab tab;
  void *dblob;            /* mdev | chain_off | chain_idx | mframe | mvel | dorg | dpre | masscom, on the device */
  double *d_shared;       /* the model's masses and centres of mass inside dblob */
  double *d_par;          /* [batch][4 nlink_model]: the instances' own (allocated by the first read-out of a batch with a table) */
  int par_gen;            /* generation of the table d_par holds (-1: none) */
  int lds_doubles;
  double *out[5];         /* R, p, v, com, comvel */
  int flags;              /* of the last launch */
  hipEvent_t done;
};

extern "C" rkfdLinks *rkfd_links_create(const rkfdModel *m, const rkfdDevModelHost *h, const rkfdDevModel *dm, int batch, char *err, int errlen)
{
#define CFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); rkfd_links_destroy( l ); return NULL; }while(0)
  rkfdLinks *l = (rkfdLinks *)calloc( 1, sizeof(rkfdLinks) );
  if( !l ){ if( err ) snprintf( err, errlen, "out of memory" ); return NULL; }
  const int NLM = m->nlink, NCH = m->nchain, NL = dm->nlink;
  l->batch = batch; l->nlink_model = NLM; l->nchain = NCH; l->par_gen = -1;
  l->lds_doubles = RKFD_LINKS_LDS_DOUBLES( NL, NLM, NCH );
  const size_t lds = sizeof(double)*(size_t)l->lds_doubles*RKFD_LINKS_WAVES;
  if( lds > 160*1024 ) CFAIL( "rkfdBatchUpdateLinks: a world of %d links in %d chains needs %zu bytes of LDS per workgroup (> 160 KiB)", NLM, NCH, lds );
  if( lds > 64*1024 && hipFuncSetAttribute( (const void *)rkfd_links_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateLinks: hipFuncSetAttribute(LDS=%zu) failed", lds );
  rkfdLinksHostTab ht;
  rkfd_links_host_build( m, h, &ht );
  const size_t ni = ht.mdev.size() + ht.chain_off.size() + ht.chain_idx.size(), ni2 = ( ni + 1 ) & ~(size_t)1;      /* (the doubles start 8-byte aligned) */
  const std::vector<double> *dv[5] = { &ht.mframe, &ht.mvel, &ht.dorg, &ht.dpre, &ht.masscom };
  size_t nd = 0, doff[5];
  for( int k=0; k<5; k++ ){ doff[k] = nd; nd += dv[k]->size(); }
  const size_t bytes = sizeof(int)*ni2 + sizeof(double)*nd;
  std::vector<char> blob( bytes );
  int *ip = (int *)blob.data();
  double *dp = (double *)( blob.data() + sizeof(int)*ni2 );
  memcpy( ip, ht.mdev.data(), sizeof(int)*ht.mdev.size() );
  memcpy( ip + ht.mdev.size(), ht.chain_off.data(), sizeof(int)*ht.chain_off.size() );
  memcpy( ip + ht.mdev.size() + ht.chain_off.size(), ht.chain_idx.data(), sizeof(int)*ht.chain_idx.size() );
  for( int k=0; k<5; k++ ) memcpy( dp + doff[k], dv[k]->data(), sizeof(double)*dv[k]->size() );
  if( hipMalloc( &l->dblob, bytes ) != hipSuccess || hipMemcpy( l->dblob, blob.data(), bytes, hipMemcpyHostToDevice ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateLinks: cannot copy the link tables to the device" );
  if( hipEventCreateWithFlags( &l->done, hipEventDisableTiming ) != hipSuccess ) CFAIL( "rkfdBatchUpdateLinks: hipEventCreate failed" );
  const int *dip = (const int *)l->dblob;
  const double *ddp = (const double *)( (const char *)l->dblob + sizeof(int)*ni2 );
  rkfdLinksTab &t = l->tab;
  t.nlink = NL; t.nlink_model = NLM; t.nchain = NCH; t.ndof = m->ndof; t.nround = dm->nround;
  t.linfo = dm->linfo; t.anc = dm->anc;
  t.mdev = dip; t.chain_off = dip + ht.mdev.size(); t.chain_idx = dip + ht.mdev.size() + ht.chain_off.size();
  t.mframe = ddp + doff[0]; t.mvel = ddp + doff[1]; t.dorg = ddp + doff[2]; t.dpre = ddp + doff[3];
  l->d_shared = (double *)ddp + doff[4];
  return l;
#undef CFAIL
}

extern "C" void rkfd_links_destroy(rkfdLinks *l)
{
  if( !l ) return;
  if( l->done ){ (void)hipEventSynchronize( l->done ); (void)hipEventDestroy( l->done ); }
  for( int k=0; k<5; k++ ) (void)hipFree( l->out[k] );
  (void)hipFree( l->d_par ); (void)hipFree( l->dblob );
  free( l );
}

extern "C" int rkfd_links_launch(rkfdLinks *l, const double *dis, const double *vel, int flags, const double *par_mass, const double *par_com,
                                 int par_gen, void *stream, char *err, int errlen)
{
  const size_t B = l->batch, NLM = l->nlink_model, NCH = l->nchain;
  const hipStream_t s = (hipStream_t)stream;
  /* the buffers the selected quantities go to: allocated once, stable afterwards */
  const size_t width[5] = { 9*NLM, 3*NLM, 6*NLM, 3*NCH, 3*NCH };
  const int need[5] = { flags & RKFD_LINKS_F_POSE, flags & RKFD_LINKS_F_POSE, flags & RKFD_LINKS_F_VEL, flags & RKFD_LINKS_F_COM, flags & RKFD_LINKS_F_COM };
  for( int k=0; k<5; k++ )
    if( need[k] && !l->out[k] ){
      const size_t n = B*width[k];
      /* (not cleared: the kernel writes every element of a selected array for every instance) */
      LHIP( hipMalloc( (void **)&l->out[k], sizeof(double)*( n ? n : 1 ) ) );
    }
  rkfdLinksTab t = l->tab;
  t.mass = l->d_shared; t.com = l->d_shared + NLM; t.par_stride = 0;
  if( ( flags & RKFD_LINKS_F_COM ) && par_mass && par_com ){
    if( par_gen != l->par_gen ){
      /* (rare: once per rkfdBatchSetParam.  An earlier read-out may still be reading the old rows) */
      LHIP( hipEventSynchronize( l->done ) );
      if( !l->d_par ) LHIP( hipMalloc( (void **)&l->d_par, sizeof(double)*( B*4*NLM + 1 ) ) );
      std::vector<double> rows( B*4*NLM + 1 );
      for( size_t i=0; i<B; i++ ){
        memcpy( &rows[i*4*NLM], par_mass + i*NLM, sizeof(double)*NLM );
        memcpy( &rows[i*4*NLM + NLM], par_com + i*3*NLM, sizeof(double)*3*NLM );
      }
      LHIP( hipMemcpy( l->d_par, rows.data(), sizeof(double)*B*4*NLM, hipMemcpyHostToDevice ) );
      l->par_gen = par_gen;
    }
    t.mass = l->d_par; t.com = l->d_par + NLM; t.par_stride = (int)( 4*NLM );
  }
  const unsigned blocks = (unsigned)( ( B + RKFD_LINKS_WAVES - 1 )/RKFD_LINKS_WAVES );
  hipLaunchKernelGGL( rkfd_links_kernel, dim3( blocks ), dim3( RKFD_WAVE*RKFD_LINKS_WAVES ), sizeof(double)*(size_t)l->lds_doubles*RKFD_LINKS_WAVES, s,
                      t, dis, vel, l->batch, flags, l->lds_doubles, l->out[0], l->out[1], l->out[2], l->out[3], l->out[4] );
  LHIP( hipGetLastError() );
  LHIP( hipEventRecord( l->done, s ) );
  l->flags = flags;
  return 0;
}

extern "C" int rkfd_links_flags(const rkfdLinks *l){ return l ? l->flags : 0; }

extern "C" int rkfd_links_get(rkfdLinks *l, double *R, double *p, double *v, double *com, double *comvel, char *err, int errlen)
{
  const size_t B = l->batch, NLM = l->nlink_model, NCH = l->nchain;
  double *dst[5] = { R, p, v, com, comvel };
  const size_t width[5] = { 9*NLM, 3*NLM, 6*NLM, 3*NCH, 3*NCH };
  LHIP( hipEventSynchronize( l->done ) );
  for( int k=0; k<5; k++ )
    if( dst[k] && B*width[k] ) LHIP( hipMemcpy( dst[k], l->out[k], sizeof(double)*B*width[k], hipMemcpyDeviceToHost ) );
  return 0;
}

extern "C" const double *rkfd_links_dev(const rkfdLinks *l, int which){ return ( l && which >= 0 && which < 5 ) ? l->out[which] : NULL; }
