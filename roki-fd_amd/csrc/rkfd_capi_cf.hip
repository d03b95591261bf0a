/* rkfd_capi_cf.hip - the contact read-out behind rkfdBatchUpdateContactForces (include/rkfd_hip.h): one kernel that computes the
 * world positions of the candidate contact vertices, the net contact wrench and contact count of every link and the generalised
 * contact force of every instance from the live joint coordinates and the candidates' flags and forces (readout/rkfd_cf.h), its
 * tables and its result buffers.  A translation unit of its own, as rkfd_capi_jac.hip is: the step kernels of rkfd_capi.hip, the
 * read-out's, the Jacobians' and the dynamics' kernels stay what they are to the instruction; this kernel's resource report goes to
 * kernel_resources_cf.txt. */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
/* (rkfd_dev_base.h's __constant__ table needs a name of its own in every translation unit: see rkfd_capi_links.hip) */
#define rkfd_kc rkfd_kc_cf
#include "readout/rkfd_cf.h"
#include "readout/rkfd_cf_host.h"

/* one instance per wavefront, `waves` of them per workgroup (4, 2 or 1 by the LDS one instance needs); every wavefront works in its
 * own piece of the workgroup's LDS and returns on its own when its instance is beyond the batch (there is no workgroup barrier) */
extern "C" __global__ void __launch_bounds__(RKFD_WAVE*RKFD_CF_MAX_WAVES)
rkfd_cf_kernel(rkfdCfTab t, const double *dis, const int *active, const double *f, int batch, int flags, int waves, int lds_doubles,
               double *opoint, double *owrench, int *ocount, double *ogenf)
{
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = LANE();
  const int wave = tid >> 6, lane = tid & ( RKFD_WAVE-1 );
  const size_t b = (size_t)blockIdx.x*waves + wave;
  if( b >= (size_t)batch ) return;
  rkfd_cf_instance( t, dis, active, f, b, lane, (double *)lds + (size_t)wave*lds_doubles, flags, opoint, owrench, ocount, ogenf );
}

#define LFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); return -1; }while(0)
#define LHIP(call) do{ hipError_t e_ = (call); if( e_ != hipSuccess ) LFAIL( "%s failed: %s", #call, hipGetErrorString( e_ ) ); }while(0)

struct rkfdCf {
  int batch, nlink, ndof, ncand;
  rkfdCfTab tab;
  void *dblob;            /* org | c_vert | parent | jtype | dofoff | cown | c_own | c_oth | l_off | l_ent, on the device */
  int lds_doubles, waves;
  void *out[4];           /* point, wrench, count (int), genf */
  int flags;              /* of the last launch */
  hipEvent_t done;
};

extern "C" rkfdCf *rkfd_cf_create(const rkfdModel *m, int batch, char *err, int errlen)
{
#define CFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); rkfd_cf_destroy( c ); return NULL; }while(0)
  rkfdCf *c = (rkfdCf *)calloc( 1, sizeof(rkfdCf) );
  if( !c ){ if( err ) snprintf( err, errlen, "out of memory" ); return NULL; }
  const int NLM = m->nlink, ND = m->ndof;
  c->batch = batch; c->nlink = NLM; c->ndof = ND; c->ncand = m->ncand;
  if( m->solver == RKFD_SOLVER_VOLUME ) CFAIL( "rkfdBatchUpdateContactForces: the Volume plugin produces no per-vertex contact forces (this world's solver is RKFD_SOLVER_VOLUME)" );
  if( ND > RKFD_WAVE ) CFAIL( "rkfdBatchUpdateContactForces: %d joint coordinates exceed the %d lanes of a wavefront", ND, RKFD_WAVE );
  c->lds_doubles = RKFD_CF_LDS_DOUBLES( NLM, ND );
  const size_t lds1 = sizeof(double)*(size_t)c->lds_doubles;
  c->waves = rkfd_cf_host_waves( lds1 );
  if( c->waves == 0 ) CFAIL( "rkfdBatchUpdateContactForces: a world of %d links and %d joint coordinates needs %zu bytes of LDS for one instance (> %d bytes a workgroup can have)", NLM, ND, lds1, RKFD_CF_HOST_LDS_MAX );
  const size_t lds = lds1*c->waves;
  if( lds > 64*1024 && hipFuncSetAttribute( (const void *)rkfd_cf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateContactForces: hipFuncSetAttribute(LDS=%zu) failed", lds );
  rkfdCfHostTab ht;
  char e2[200] = "";
  if( rkfd_cf_host_build( m, 0, NULL, NULL, NULL, &ht, e2, sizeof(e2) ) < 0 ) CFAIL( "rkfdBatchUpdateContactForces: %s", e2 );
  /* one blob: the doubles first, then the ints */
  const size_t nl1 = NLM > 0 ? NLM : 1;
  const size_t nd = 12*nl1 + ht.c_vert.size();
  const size_t ni = 3*nl1 + ht.cown.size() + ht.c_own.size() + ht.c_oth.size() + ht.l_off.size() + ht.l_ent.size();
  const size_t bytes = sizeof(double)*nd + sizeof(int)*ni;
  std::vector<char> blob( bytes, 0 );
  double *dp = (double *)blob.data();
  int *ip = (int *)( blob.data() + sizeof(double)*nd );
  const size_t o_org = 0, o_cv = 12*nl1;
  const size_t o_par = 0, o_jt = nl1, o_off = 2*nl1, o_cown = 3*nl1, o_own = o_cown + ht.cown.size(), o_oth = o_own + ht.c_own.size(),
               o_lo = o_oth + ht.c_oth.size(), o_le = o_lo + ht.l_off.size();
  memcpy( dp + o_org, m->org, sizeof(double)*12*NLM );
  memcpy( dp + o_cv, ht.c_vert.data(), sizeof(double)*ht.c_vert.size() );
  memcpy( ip + o_par, m->parent, sizeof(int)*NLM ); memcpy( ip + o_jt, m->jtype, sizeof(int)*NLM ); memcpy( ip + o_off, m->dofoff, sizeof(int)*NLM );
  memcpy( ip + o_cown, ht.cown.data(), sizeof(int)*ht.cown.size() );
  memcpy( ip + o_own, ht.c_own.data(), sizeof(int)*ht.c_own.size() ); memcpy( ip + o_oth, ht.c_oth.data(), sizeof(int)*ht.c_oth.size() );
  memcpy( ip + o_lo, ht.l_off.data(), sizeof(int)*ht.l_off.size() ); memcpy( ip + o_le, ht.l_ent.data(), sizeof(int)*ht.l_ent.size() );
  if( hipMalloc( &c->dblob, bytes ) != hipSuccess || hipMemcpy( c->dblob, blob.data(), bytes, hipMemcpyHostToDevice ) != hipSuccess )
    CFAIL( "rkfdBatchUpdateContactForces: cannot copy the model tables to the device" );
  if( hipEventCreateWithFlags( &c->done, hipEventDisableTiming ) != hipSuccess ) CFAIL( "rkfdBatchUpdateContactForces: hipEventCreate failed" );
  const double *ddp = (const double *)c->dblob;
  const int *dip = (const int *)( (const char *)c->dblob + sizeof(double)*nd );
  rkfdCfTab &t = c->tab;
  memset( &t, 0, sizeof(t) );
  t.j.nlink = NLM; t.j.nchain = m->nchain; t.j.ndof = ND; t.j.nsite = 0;
  t.j.parent = dip + o_par; t.j.jtype = dip + o_jt; t.j.dofoff = dip + o_off; t.j.cown = dip + o_cown; t.j.org = ddp + o_org;
  t.ncand = ht.ncand;
  t.c_own = dip + o_own; t.c_oth = dip + o_oth; t.c_vert = ddp + o_cv; t.l_off = dip + o_lo; t.l_ent = dip + o_le;
  return c;
#undef CFAIL
}

extern "C" void rkfd_cf_destroy(rkfdCf *c)
{
  if( !c ) return;
  if( c->done ){ (void)hipEventSynchronize( c->done ); (void)hipEventDestroy( c->done ); }
  for( int k=0; k<4; k++ ) (void)hipFree( c->out[k] );
  (void)hipFree( c->dblob );
  free( c );
}

static void cf_widths(const rkfdCf *c, size_t *bytes)
{
  const size_t B = c->batch;
  bytes[0] = sizeof(double)*B*c->ncand*3; bytes[1] = sizeof(double)*B*c->nlink*6; bytes[2] = sizeof(int)*B*c->nlink; bytes[3] = sizeof(double)*B*c->ndof;
}

extern "C" int rkfd_cf_launch(rkfdCf *c, const double *dis, const int *active, const double *f, int flags, void *stream, char *err, int errlen)
{
  const hipStream_t s = (hipStream_t)stream;
  /* the buffers the selected quantities go to: allocated once, stable afterwards */
  size_t bytes[4];
  cf_widths( c, bytes );
  const int need[4] = { flags & RKFD_CF_F_POINT, flags & RKFD_CF_F_WRENCH, flags & RKFD_CF_F_WRENCH, flags & RKFD_CF_F_GENF };
  for( int k=0; k<4; k++ )
    if( need[k] && !c->out[k] ){
      /* (not cleared: the kernel writes every element of a selected array for every instance) */
      LHIP( hipMalloc( &c->out[k], bytes[k] ? bytes[k] : 8 ) );
    }
  const unsigned blocks = (unsigned)( ( (size_t)c->batch + c->waves - 1 )/c->waves );
  hipLaunchKernelGGL( rkfd_cf_kernel, dim3( blocks ), dim3( RKFD_WAVE*c->waves ), sizeof(double)*(size_t)c->lds_doubles*c->waves, s,
                      c->tab, dis, active, f, c->batch, flags, c->waves, c->lds_doubles,
                      (double *)c->out[0], (double *)c->out[1], (int *)c->out[2], (double *)c->out[3] );
  LHIP( hipGetLastError() );
  LHIP( hipEventRecord( c->done, s ) );
  c->flags = flags;
  return 0;
}

extern "C" int rkfd_cf_flags(const rkfdCf *c){ return c ? c->flags : 0; }

extern "C" int rkfd_cf_get(rkfdCf *c, double *point, double *wrench, int *count, double *genf, char *err, int errlen)
{
  void *dst[4] = { point, wrench, count, genf };
  size_t bytes[4];
  cf_widths( c, bytes );
  LHIP( hipEventSynchronize( c->done ) );
  for( int k=0; k<4; k++ )
    if( dst[k] && bytes[k] ) LHIP( hipMemcpy( dst[k], c->out[k], bytes[k], hipMemcpyDeviceToHost ) );
  return 0;
}

extern "C" const void *rkfd_cf_dev(const rkfdCf *c, int which){ return ( c && which >= 0 && which < 4 ) ? c->out[which] : NULL; }
