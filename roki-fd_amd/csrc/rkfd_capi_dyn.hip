/* rkfd_capi_dyn.hip - the joint-space dynamics behind rkfdBatchUpdateDynamics (include/rkfd_hip.h): one kernel that computes the
 * joint-space inertia matrix, the bias force and the gravity force of every instance from the live joint state (readout/rkfd_dyn.h),
 * its tables and its result buffers.  A translation unit of its own, as rkfd_capi_jac.hip is: the step kernels of rkfd_capi.hip, the
 * read-out's and the Jacobians' kernels stay what they are to the instruction; this kernel's resource report goes to
 * kernel_resources_dyn.txt. */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
/* (rkfd_dev_base.h's __constant__ table needs a name of its own in every translation unit: see rkfd_capi_links.hip) */
#define rkfd_kc rkfd_kc_dyn
#include "readout/rkfd_dyn.h"
#include "readout/rkfd_dyn_host.h"

/* one instance per wavefront, `waves` of them per workgroup (4, 2 or 1 by the LDS one instance needs); every wavefront works in its
 * own piece of the workgroup's LDS and returns on its own when its instance is beyond the batch (there is no workgroup barrier) */
extern "C" __global__ void __launch_bounds__(RKFD_WAVE*RKFD_DYN_MAX_WAVES)
rkfd_dyn_kernel(rkfdDynTab t, const double *dis, const double *vel, int batch, int flags, int waves, int lds_doubles, double *oM, double *oh, double *og)
{
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = LANE();
  const int wave = tid >> 6, lane = tid & ( RKFD_WAVE-1 );
  const size_t b = (size_t)blockIdx.x*waves + wave;
  if( b >= (size_t)batch ) return;
  rkfd_dyn_instance( t, dis, vel, b, lane, (double *)lds + (size_t)wave*lds_doubles, flags, oM, oh, og );
}

#define LFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); return -1; }while(0)
#define LHIP(call) do{ hipError_t e_ = (call); if( e_ != hipSuccess ) LFAIL( "%s failed: %s", #call, hipGetErrorString( e_ ) ); }while(0)

struct rkfdDyn {
  int batch, nlink, ndof;
  rkfdDynTab tab;
  void *dblob;            /* amask | rotor | org | mass, com, inertia | parent | jtype | dofoff | cown | level and child lists, on the device */
  double *d_shared;       /* the model's masses, centres of mass and inertias inside dblob */
  double *d_par;          /* [batch][13 nlink]: the instances' own (allocated by the first launch of a batch with a table) */
  int par_gen;            /* generation of the table d_par holds (-1: none) */
  int lds_doubles, waves;
  double *out[3];         /* M, h, g */
  int flags;              /* of the last launch */
  hipEvent_t done;
};

extern "C" rkfdDyn *rkfd_dyn_create(const rkfdModel *m, int batch, char *err, int errlen)
{
#define CFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); rkfd_dyn_destroy( d ); return NULL; }while(0)
  rkfdDyn *d = (rkfdDyn *)calloc( 1, sizeof(rkfdDyn) );
  if( !d ){ if( err ) snprintf( err, errlen, "out of memory" ); return NULL; }
  const int NLM = m->nlink, ND = m->ndof;
  d->batch = batch; d->nlink = NLM; d->ndof = ND; d->par_gen = -1;
  if( ND > RKFD_WAVE ) CFAIL( "rkfdBatchUpdateDynamics: %d joint coordinates exceed the %d lanes of a wavefront", ND, RKFD_WAVE );
  d->lds_doubles = RKFD_DYN_LDS_DOUBLES( NLM, ND );
  const size_t lds1 = sizeof(double)*(size_t)d->lds_doubles;
  d->waves = rkfd_dyn_host_waves( lds1 );
  if( d->waves == 0 ) CFAIL( "rkfdBatchUpdateDynamics: a world of %d links and %d joint coordinates needs %zu bytes of LDS for one instance (> %d bytes a workgroup can have)", NLM, ND, lds1, RKFD_DYN_HOST_LDS_MAX );
  const size_t lds = lds1*d->waves;
  if( lds > 64*1024 && hipFuncSetAttribute( (const void *)rkfd_dyn_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateDynamics: hipFuncSetAttribute(LDS=%zu) failed", lds );
  rkfdDynHostTab ht;
  rkfd_dyn_host_build( m, &ht );
  /* one blob: the 8-byte tables first, then the ints */
  const size_t nl1 = NLM > 0 ? NLM : 1;
  const size_t n8 = ht.amask.size() + ht.rotor.size() + 12*nl1 + ht.mci.size();
  const size_t ni = 3*nl1 + ht.cown.size() + ht.lev_off.size() + ht.lev_idx.size() + ht.child_off.size() + ht.child_idx.size();
  const size_t bytes = 8*n8 + sizeof(int)*ni;
  std::vector<char> blob( bytes, 0 );
  unsigned long long *up = (unsigned long long *)blob.data();
  double *dp = (double *)( up + ht.amask.size() );
  int *ip = (int *)( blob.data() + 8*n8 );
  const size_t o_rot = 0, o_org = ht.rotor.size(), o_mci = o_org + 12*nl1;
  const size_t o_par = 0, o_jt = nl1, o_off = 2*nl1, o_own = 3*nl1, o_lo = o_own + ht.cown.size(), o_li = o_lo + ht.lev_off.size(),
               o_co = o_li + ht.lev_idx.size(), o_ci = o_co + ht.child_off.size();
  memcpy( up, ht.amask.data(), 8*ht.amask.size() );
  memcpy( dp + o_rot, ht.rotor.data(), sizeof(double)*ht.rotor.size() );
  memcpy( dp + o_org, m->org, sizeof(double)*12*NLM );
  memcpy( dp + o_mci, ht.mci.data(), sizeof(double)*ht.mci.size() );
  memcpy( ip + o_par, m->parent, sizeof(int)*NLM ); memcpy( ip + o_jt, m->jtype, sizeof(int)*NLM ); memcpy( ip + o_off, m->dofoff, sizeof(int)*NLM );
  memcpy( ip + o_own, ht.cown.data(), sizeof(int)*ht.cown.size() );
  memcpy( ip + o_lo, ht.lev_off.data(), sizeof(int)*ht.lev_off.size() ); memcpy( ip + o_li, ht.lev_idx.data(), sizeof(int)*ht.lev_idx.size() );
  memcpy( ip + o_co, ht.child_off.data(), sizeof(int)*ht.child_off.size() ); memcpy( ip + o_ci, ht.child_idx.data(), sizeof(int)*ht.child_idx.size() );
  if( hipMalloc( &d->dblob, bytes ) != hipSuccess || hipMemcpy( d->dblob, blob.data(), bytes, hipMemcpyHostToDevice ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateDynamics: cannot copy the model tables to the device" );
  if( hipEventCreateWithFlags( &d->done, hipEventDisableTiming ) != hipSuccess ) CFAIL( "rkfdBatchUpdateDynamics: hipEventCreate failed" );
  const unsigned long long *dup = (const unsigned long long *)d->dblob;
  const double *ddp = (const double *)( dup + ht.amask.size() );
  const int *dip = (const int *)( (const char *)d->dblob + 8*n8 );
  rkfdDynTab &t = d->tab;
  t.nlink = NLM; t.ndof = ND; t.nlevel = ht.nlevel;
  t.parent = dip + o_par; t.jtype = dip + o_jt; t.dofoff = dip + o_off; t.cown = dip + o_own;
  t.lev_off = dip + o_lo; t.lev_idx = dip + o_li; t.child_off = dip + o_co; t.child_idx = dip + o_ci;
  t.amask = dup; t.rotor = ddp + o_rot; t.org = ddp + o_org;
  d->d_shared = (double *)ddp + o_mci;
  return d;
#undef CFAIL
}

extern "C" void rkfd_dyn_destroy(rkfdDyn *d)
{
  if( !d ) return;
  if( d->done ){ (void)hipEventSynchronize( d->done ); (void)hipEventDestroy( d->done ); }
  for( int k=0; k<3; k++ ) (void)hipFree( d->out[k] );
  (void)hipFree( d->d_par ); (void)hipFree( d->dblob );
  free( d );
}

extern "C" int rkfd_dyn_launch(rkfdDyn *d, const double *dis, const double *vel, int flags, const double *par_mass, const double *par_com,
                               const double *par_inertia, int par_gen, void *stream, char *err, int errlen)
{
  const size_t B = d->batch, NLM = d->nlink, ND = d->ndof;
  const hipStream_t s = (hipStream_t)stream;
  /* the buffers the selected quantities go to: allocated once, stable afterwards */
  const size_t width[3] = { ND*ND, ND, ND };
  const int need[3] = { flags & RKFD_DYN_F_MASS, flags & RKFD_DYN_F_BIAS, flags & RKFD_DYN_F_GRAVITY };
  for( int k=0; k<3; k++ )
    if( need[k] && !d->out[k] ){
      const size_t n = B*width[k];
      /* (not cleared: the kernel writes every element of a selected array for every instance) */
      LHIP( hipMalloc( (void **)&d->out[k], sizeof(double)*( n ? n : 1 ) ) );
    }
  rkfdDynTab t = d->tab;
  t.mass = d->d_shared; t.com = d->d_shared + NLM; t.inertia = d->d_shared + 4*NLM; t.par_stride = 0;
  if( par_mass && par_com && par_inertia ){
    if( par_gen != d->par_gen ){
      /* (rare: once per rkfdBatchSetParam.  An earlier launch may still be reading the old rows) */
      LHIP( hipEventSynchronize( d->done ) );
      if( !d->d_par ) LHIP( hipMalloc( (void **)&d->d_par, sizeof(double)*( B*13*NLM + 1 ) ) );
      std::vector<double> rows;
      rkfd_dyn_host_rows( d->nlink, B, par_mass, par_com, par_inertia, &rows );
      LHIP( hipMemcpy( d->d_par, rows.data(), sizeof(double)*B*13*NLM, hipMemcpyHostToDevice ) );
      d->par_gen = par_gen;
    }
    t.mass = d->d_par; t.com = d->d_par + NLM; t.inertia = d->d_par + 4*NLM; t.par_stride = (int)( 13*NLM );
  }
  const unsigned blocks = (unsigned)( ( B + d->waves - 1 )/d->waves );
  hipLaunchKernelGGL( rkfd_dyn_kernel, dim3( blocks ), dim3( RKFD_WAVE*d->waves ), sizeof(double)*(size_t)d->lds_doubles*d->waves, s,
                      t, dis, vel, d->batch, flags, d->waves, d->lds_doubles, d->out[0], d->out[1], d->out[2] );
  LHIP( hipGetLastError() );
  LHIP( hipEventRecord( d->done, s ) );
  d->flags = flags;
  return 0;
}

extern "C" int rkfd_dyn_flags(const rkfdDyn *d){ return d ? d->flags : 0; }

extern "C" int rkfd_dyn_get(rkfdDyn *d, double *M, double *h, double *g, char *err, int errlen)
{
  const size_t B = d->batch, ND = d->ndof;
  double *dst[3] = { M, h, g };
  const size_t width[3] = { ND*ND, ND, ND };
  LHIP( hipEventSynchronize( d->done ) );
  for( int k=0; k<3; k++ )
    if( dst[k] && B*width[k] ) LHIP( hipMemcpy( dst[k], d->out[k], sizeof(double)*B*width[k], hipMemcpyDeviceToHost ) );
  return 0;
}

extern "C" const double *rkfd_dyn_dev(const rkfdDyn *d, int which){ return ( d && which >= 0 && which < 3 ) ? d->out[which] : NULL; }
