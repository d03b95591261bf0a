/* rkfd_capi.hip - C ABI (include/rkfd_hip.h) over the gfx950 kernel in rkfd_device.h. */
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#ifndef _GNU_SOURCE
#define _GNU_SOURCE
#endif
#include <dlfcn.h>
#include <link.h>
#include <pthread.h>
#include <unistd.h>
#include <sys/stat.h>
#include <string>
#include <vector>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "rkfd_hip.h"
#include "rkfd_device.h"
#include "rkfd_devmodel_host.h"
#include "readout/rkfd_links_host.h"   /* the task-space read-out (rkfd_capi_links.hip) */
#include "readout/rkfd_jac_host.h"     /* the task-space Jacobians (rkfd_capi_jac.hip) */
#include "readout/rkfd_dyn_host.h"     /* the joint-space dynamics (rkfd_capi_dyn.hip) */
#include "readout/rkfd_cf_host.h"      /* the contact read-out (rkfd_capi_cf.hip) */
#include "reset/rkfd_reset_host.h"     /* the per-instance reset and its bank of start states (rkfd_capi_reset.hip) */
#include "rkfd_device_src.inc"       /* the device headers as string literals (tools/embed_sources.py), for hipRTC */

static thread_local char g_err[512] = "";
#define SETERR(...) snprintf( g_err, sizeof(g_err), __VA_ARGS__ )
#define HIPCHK(call, ret) do{ hipError_t e_ = (call); if( e_ != hipSuccess ){ \
  SETERR( "%s failed: %s", #call, hipGetErrorString( e_ ) ); return ret; } }while(0)

/* Per-instance physical parameters (rkfdBatchSetParam): a batch that carries a table launches a SECOND set of step kernels, the same
 * device code compiled with RKFD_PARAMS = 1 (rkfd_capi_par.hip, a translation unit of its own; the world-specific kernel likewise),
 * which take the doubles of one table row as a ninth argument and read the parameters at the instance's row (RKFD_PAR in
 * rkfd_dev_base.h); the model `m` such a launch passes has its mass .. sfric and ci_sf .. ci_v pointing at the table's first row
 * (par_model below).  The kernels of this file are what they were before the table existed, instruction for instruction: a batch
 * without a table pays nothing for the feature. */
/* one workgroup = one wavefront = one world instance; state lives in LDS for the whole launch.
 * Register budget: the kernels need ~150-160 VGPRs when built with -mllvm -disable-machine-licm (see Makefile):
 * three waves per SIMD, i.e. up to twelve instances per CU where the LDS allows (10 for the humanoid worlds).
 * With machine LICM on, the backend hoists ~35 registers of literals (sincos polynomial coefficients, fp64
 * constants) and addresses out of the step loop and the kernels need 184-193. */
#define RKFD_KERNEL(name, prof, vqp, pk, waves) \
extern "C" __global__ void __launch_bounds__(RKFD_WAVE, waves) \
name(rkfdDevModel m, rkfdDevState st, int first, int mode, int nsteps, int *errflag, const double *ctrl, int ctrl_stride) \
{ \
  extern __shared__ __attribute__((aligned(16))) char lds[]; \
  const int b = first + (int)blockIdx.x; \
  if( b >= st.batch ) return; \
  rkfd_instance<prof, vqp, pk>( m, st, b, lds, mode, nsteps, errflag, true, 0, prof ? nullptr : ctrl, ctrl_stride ); \
}
RKFD_KERNEL( rkfd_step_kernel, false, 0, false, 3 )
/* the contact matrix as a packed lower triangle (worlds where that lets one more instance share a CU) */
RKFD_KERNEL( rkfd_step_kernel_pk, false, 0, true, 3 )
/* the variant that also carries the Vert plugin's QP (worlds with rigid pairs under the Vert plugin);
 * kept apart so that its code and registers do not weigh on the MLCP / penalty kernel */
/* (two waves per SIMD: up to 24 unknowns the QP keeps the factor of its Q in registers - 96 of them - and the QP's LDS allows at
 *  most eight instances per CU anyway) */
RKFD_KERNEL( rkfd_step_kernel_vqp, false, 1, false, 2 )
/* diagnostic instantiations with in-kernel phase stamps (rkfdBatchProfile); they never carry a control schedule (the profile steps
 * with the batch's motor input), so they drop it and keep their registers */
RKFD_KERNEL( rkfd_step_kernel_prof, true, 0, false, 3 )
RKFD_KERNEL( rkfd_step_kernel_prof_pk, true, 0, true, 3 )
RKFD_KERNEL( rkfd_step_kernel_prof_vqp, true, 1, false, 2 )
/* the variant that carries the Volume plugin (worlds with rigid pairs under it).  Built for two waves per SIMD: the phase is
 * latency-bound (a dozen lanes at work, dependent LDS / readlane chains), so a second wave per SIMD is worth more than the
 * ~90 vector registers it spills (measured, box on the floor / humanoid on two soles, M steps/s: one wave 2.33 / 1.49, two
 * 4.55 / 1.68, three 4.47 / 1.41 - the humanoid's 32 KB of LDS allow five instances per CU either way) */
extern "C" __global__ void __launch_bounds__(RKFD_WAVE, 2)
rkfd_step_kernel_vol(rkfdDevModel m, rkfdDevState st, int first, int mode, int nsteps, int *errflag, const double *ctrl, int ctrl_stride)
{
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int b = first + (int)blockIdx.x;
  if( b >= st.batch ) return;
  rkfd_instance<false, 2, false>( m, st, b, lds, mode, nsteps, errflag, true, 0, ctrl, ctrl_stride );
}
extern "C" __global__ void __launch_bounds__(RKFD_WAVE, 2)
rkfd_step_kernel_prof_vol(rkfdDevModel m, rkfdDevState st, int first, int mode, int nsteps, int *errflag, const double *ctrl, int ctrl_stride)
{
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int b = first + (int)blockIdx.x;
  if( b >= st.batch ) return;
  rkfd_instance<true, 2, false>( m, st, b, lds, mode, nsteps, errflag, true, 0, nullptr, ctrl_stride );
}

/* rkfdBatchRestore: one workgroup copies one instance's state rows back from the snapshot */
extern "C" __global__ void __launch_bounds__(RKFD_WAVE)
rkfd_restore_kernel(rkfdDevState st, rkfdDevState sn, int first, int ND, int NLM, int NC)
{
  const size_t b = (size_t)first + blockIdx.x;
  if( b >= (size_t)st.batch ) return;
  for( int j=threadIdx.x; j<ND; j+=RKFD_WAVE ){
    st.dis[b*ND+j] = sn.dis[b*ND+j]; st.vel[b*ND+j] = sn.vel[b*ND+j]; st.acc[b*ND+j] = sn.acc[b*ND+j];
  }
  for( int j=threadIdx.x; j<NLM; j+=RKFD_WAVE ){
    st.piv_type[b*NLM+j] = sn.piv_type[b*NLM+j]; st.piv_prev[b*NLM+j] = sn.piv_prev[b*NLM+j];
    st.brk[b*NLM+j] = sn.brk[b*NLM+j];
  }
  for( int j=threadIdx.x; j<NC; j+=RKFD_WAVE ){
    st.cv_active[b*NC+j] = sn.cv_active[b*NC+j]; st.cv_type[b*NC+j] = sn.cv_type[b*NC+j];
  }
  for( int j=threadIdx.x; j<3*NC; j+=RKFD_WAVE ){
    st.cv_ref[b*3*NC+j] = sn.cv_ref[b*3*NC+j]; st.cv_f[b*3*NC+j] = sn.cv_f[b*3*NC+j];
  }
}

typedef void (*rkfdKernel)(rkfdDevModel, rkfdDevState, int, int, int, int *, const double *, int);
typedef void (*rkfdKernelPar)(rkfdDevModel, rkfdDevState, int, int, int, int *, const double *, int, int);
/* rkfd_capi_par.hip: the step kernel built with RKFD_PARAMS = 1 - kind 0 plain, 1 packed matrix, 2 Vert QP, 3 Volume */
extern "C" rkfdKernelPar rkfd_par_kernel(int kind, int prof);
#define RKFD_MAX_SPLIT 8

struct rkfdBatch {
  int device, batch, nlink, ndof, ncand;
  rkfdDevModelHost host;
  rkfdDevModel dm;        /* device-pointer version */
  void *dblob;
  rkfdDevState st;
  rkfdDevState snap;      /* rkfdBatchSnapshot: device-resident copy of the state (allocated on first use) */
  int has_snap;
  int *d_err;
  size_t lds_bytes;
  size_t lds_pad;         /* RKFD_LDS_PAD_BYTES (diagnostic): extra LDS every workgroup asks for, one instance per wavefront or two */
  rkfdKernel kern, kern_prof;
  rkfdKernelPar kern_par, kern_prof_par;      /* the same with a table of per-instance parameters */
  /* rkfdBatchSpecialize: the step kernel compiled for this world (hipRTC); NULL = the generic kernels above */
  hipModule_t spec_mod;
  hipFunction_t spec_fn;
  hipStream_t last_stream;   /* the caller's stream of the last launch: what the synchronous accessors wait for besides the internal streams */
  int launched;              /* work went to last_stream that no accessor has waited for yet */
  int spec_par;              /* 1: spec_fn was compiled with RKFD_PARAMS = 1 (the batch carried a table when it was made) */
  /* rkfdBatchSetInstancesPerWave( b, 2 ): a second device model (sweep schedule with four links per iteration) for the
   * world-specific kernel built with RKFD_W = 2 - two instances per wavefront, 32 lanes each */
  int steps_per_launch;      /* under split launches: steps one launch carries (rkfdBatchSetStepsPerLaunch) */
  int ipw;                           /* instances per wavefront of the specialised kernel: 1 or 2 */
  const rkfdModel *model_for_w2;     /* the caller's model (must outlive the batch, as for rkfdBatchCreate's own use) */
  rkfdDevModelHost host2;
  rkfdDevModel dm2;
  void *dblob2;
  /* split launches (rkfdBatchSetSplit): the batch goes out as nsplit kernels on internal streams, so that the
   * tail of one step of one part overlaps the next step of another (the instances are independent) */
  int nsplit;
  hipStream_t sub[RKFD_MAX_SPLIT];
  hipEvent_t fork, done[RKFD_MAX_SPLIT];
  int pending;                       /* work on the internal streams that no stream has been joined with yet */
  /* optional per-launch timing (rkfdBatchTimeLaunches) */
  int timing;
  std::vector<hipEvent_t> *tev;      /* pool of pre-created events; start / stop pairs occupy [0, tused) */
  size_t tused;
  /* rkfdBatchUpdateControlled: the schedule's device copy and its pinned host staging (grown on demand); every part copies its own
   * block on the stream it steps on, and ctrl_ev[k] marks the end of part k's copy: the next call waits for them before it
   * overwrites the staging */
  double *d_ctrl, *h_ctrl;
  size_t ctrl_cap;                   /* doubles */
  hipEvent_t ctrl_ev[RKFD_MAX_SPLIT];
  int ctrl_nev;                      /* events of ctrl_ev recorded by the last call */
  /* rkfdBatchSetParam: the host copy in MODEL space, h_par[key][batch][width] (allocated by the first Set, initialised from the
   * model), and the device table rebuilt from it on every Set: one contiguous row of par_stride doubles per instance, the device
   * links' mass | com | inertia | stiff | visc | coulomb | sfric, then ci_sf .. ci_v (rkfd_devmodel_par_row).  d_par == NULL: no table */
  double *h_par[RKFD_PAR_COUNT];
  double *d_par;
  int par_stride;
  /* rkfdBatchUpdateLinks: the task-space read-out's tables and result buffers (rkfd_capi_links.hip), made by the first read-out -
   * a batch that never asks has none; par_gen counts the changes of the parameter table (the read-out keeps model-space rows of its own) */
  rkfdLinks *links;
  int par_gen;
  /* rkfdBatchSetJacobianSites / UpdateJacobians: the Jacobians' tables, sites and result buffers (rkfd_capi_jac.hip), made by the
   * first of those calls - a batch that never asks has none */
  rkfdJac *jac;
  /* rkfdBatchUpdateDynamics: the joint-space dynamics' tables and result buffers (rkfd_capi_dyn.hip), made by the first launch - a
   * batch that never asks has none */
  rkfdDyn *dyn;
  /* rkfdBatchUpdateContactForces[Dev]: the contact read-out's tables and result buffers (rkfd_capi_cf.hip), made by the first launch -
   * a batch that never asks has none */
  rkfdCf *cf;
  /* rkfdBatchBankReserve / rkfdBatchReset: the bank of start states and the staging of the slot values (rkfd_capi_reset.hip), made by
   * the first of those calls - a batch that never resets one instance alone has none */
  rkfdReset *reset;
};

extern "C" const char *rkfdHipLastError(void){ return g_err; }

extern "C" int rkfdHipDeviceCount(void)
{
  int n = 0;
  if( hipGetDeviceCount( &n ) != hipSuccess ) return 0;
  return n;
}

template<class T> static int dalloc(T **p, size_t n)
{
  hipError_t e = hipMalloc( (void **)p, sizeof(T)*( n ? n : 1 ) );
  if( e != hipSuccess ){ SETERR( "hipMalloc(%zu bytes) failed: %s", sizeof(T)*n, hipGetErrorString( e ) ); return -1; }
  e = hipMemset( *p, 0, sizeof(T)*( n ? n : 1 ) );
  if( e != hipSuccess ){ SETERR( "hipMemset failed: %s", hipGetErrorString( e ) ); return -1; }
  return 0;
}

extern "C" rkfdBatch *rkfdBatchCreate(const rkfdModel *m, int batch, int device, int max_rigid)
{
  if( !m || batch < 1 ){ SETERR( "rkfdBatchCreate: bad arguments" ); return NULL; }
  int ndev = 0;
  if( hipGetDeviceCount( &ndev ) != hipSuccess || ndev == 0 ){
    SETERR( "rkfdBatchCreate: no HIP device available (the MI355X path has no CPU fallback)" );
    return NULL;
  }
  if( device < 0 || device >= ndev ){ SETERR( "rkfdBatchCreate: device %d out of range (%d visible)", device, ndev ); return NULL; }
  HIPCHK( hipSetDevice( device ), NULL );

  rkfdBatch *b = (rkfdBatch *)calloc( 1, sizeof(rkfdBatch) );
  if( b ){ b->nsplit = 1; b->steps_per_launch = 5; b->tev = new std::vector<hipEvent_t>(); }
  if( !b ){ SETERR( "out of memory" ); return NULL; }
  char err[256];
  if( rkfd_devmodel_build( m, max_rigid, &b->host, err, sizeof(err) ) < 0 ){
    SETERR( "rkfdBatchCreate: %s", err );
    rkfdBatchDestroy( b );
    return NULL;
  }
  b->device = device; b->batch = batch; b->nlink = m->nlink; b->ndof = m->ndof; b->ncand = m->ncand;
  b->lds_bytes = b->host.lds_bytes;
  /* diagnostic (tools/sweep_residency.sh): ask for more LDS than needed, to measure throughput against residency */
  if( const char *pad = getenv( "RKFD_LDS_PAD_BYTES" ) ) b->lds_pad = (size_t)( atoi( pad ) > 0 ? atoi( pad ) : 0 );
  b->lds_bytes += b->lds_pad;
  if( b->lds_bytes > 160*1024 ){
    SETERR( "rkfdBatchCreate: one instance needs %zu bytes of LDS (> 160 KiB)", b->lds_bytes );
    rkfdBatchDestroy( b );
    return NULL;
  }
  if( hipMalloc( &b->dblob, b->host.bytes ) != hipSuccess ||
      hipMemcpy( b->dblob, b->host.blob, b->host.bytes, hipMemcpyHostToDevice ) != hipSuccess ){
    SETERR( "rkfdBatchCreate: cannot copy the model to the device" );
    rkfdBatchDestroy( b );
    return NULL;
  }
  b->dm = b->host.dm;
  rkfd_devmodel_rebase( &b->dm, b->host.blob, b->dblob );
  b->ipw = 1; b->model_for_w2 = m;

  const size_t B = batch, ND = m->ndof, NL = m->nlink, NC = m->ncand;
  int bad = 0;
  bad |= dalloc( &b->st.dis, B*ND ); bad |= dalloc( &b->st.vel, B*ND ); bad |= dalloc( &b->st.acc, B*ND );
  bad |= dalloc( &b->st.motor_in, B*NL ); bad |= dalloc( &b->st.piv_type, B*NL ); bad |= dalloc( &b->st.piv_prev, B*NL );
  bad |= dalloc( &b->st.brk, B*NL );
  bad |= dalloc( &b->st.cv_active, B*NC ); bad |= dalloc( &b->st.cv_type, B*NC );
  bad |= dalloc( &b->st.cv_ref, B*NC*3 ); bad |= dalloc( &b->st.cv_f, B*NC*3 );
  bad |= dalloc( &b->st.stat, B*4 );
  bad |= dalloc( &b->d_err, 1 );
  b->st.dbg = NULL; b->st.dbg_stride = 0; b->st.batch = batch; b->st.prof = NULL;
  if( bad ){ rkfdBatchDestroy( b ); return NULL; }
  b->kern = b->dm.vert_rigid ? rkfd_step_kernel_vqp : ( b->dm.ma_packed ? rkfd_step_kernel_pk : rkfd_step_kernel );
  b->kern_prof = b->dm.vert_rigid ? rkfd_step_kernel_prof_vqp : ( b->dm.ma_packed ? rkfd_step_kernel_prof_pk : rkfd_step_kernel_prof );
  if( b->dm.vol_np > 0 ){ b->kern = rkfd_step_kernel_vol; b->kern_prof = rkfd_step_kernel_prof_vol; }
  {
    const int kind = b->dm.vol_np > 0 ? 3 : ( b->dm.vert_rigid ? 2 : ( b->dm.ma_packed ? 1 : 0 ) );
    b->kern_par = rkfd_par_kernel( kind, 0 ); b->kern_prof_par = rkfd_par_kernel( kind, 1 );
  }
  if( b->lds_bytes > 64*1024 ){
    hipError_t e = hipFuncSetAttribute( (const void *)b->kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->lds_bytes );
    if( e == hipSuccess ) e = hipFuncSetAttribute( (const void *)b->kern_prof, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->lds_bytes );
    if( e == hipSuccess ) e = hipFuncSetAttribute( (const void *)b->kern_par, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->lds_bytes );
    if( e == hipSuccess ) e = hipFuncSetAttribute( (const void *)b->kern_prof_par, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b->lds_bytes );
    if( e != hipSuccess ){ SETERR( "hipFuncSetAttribute(LDS=%zu) failed: %s", b->lds_bytes, hipGetErrorString( e ) ); rkfdBatchDestroy( b ); return NULL; }
  }
  return b;
}

extern "C" void rkfdBatchDestroy(rkfdBatch *b)
{
  if( !b ) return;
  (void)hipFree( b->st.dis ); (void)hipFree( b->st.vel ); (void)hipFree( b->st.acc );
  (void)hipFree( b->st.motor_in ); (void)hipFree( b->st.piv_type ); (void)hipFree( b->st.piv_prev ); (void)hipFree( b->st.brk );
  (void)hipFree( b->st.cv_active ); (void)hipFree( b->st.cv_type ); (void)hipFree( b->st.cv_ref ); (void)hipFree( b->st.cv_f );
  (void)hipFree( b->st.stat );
  (void)hipFree( b->snap.dis ); (void)hipFree( b->snap.vel ); (void)hipFree( b->snap.acc );
  (void)hipFree( b->snap.piv_type ); (void)hipFree( b->snap.piv_prev ); (void)hipFree( b->snap.brk );
  (void)hipFree( b->snap.cv_active ); (void)hipFree( b->snap.cv_type ); (void)hipFree( b->snap.cv_ref ); (void)hipFree( b->snap.cv_f );
  if( b->fork ){
    (void)hipEventDestroy( b->fork );
    for( int k=0; k<RKFD_MAX_SPLIT; k++ ){ (void)hipStreamSynchronize( b->sub[k] ); (void)hipStreamDestroy( b->sub[k] ); (void)hipEventDestroy( b->done[k] ); }
  }
  if( b->tev ){ for( size_t i=0; i<b->tev->size(); i++ ) (void)hipEventDestroy( (*b->tev)[i] ); delete b->tev; }
  for( int k=0; k<b->ctrl_nev; k++ ) (void)hipEventSynchronize( b->ctrl_ev[k] );
  for( int k=0; k<RKFD_MAX_SPLIT; k++ ) if( b->ctrl_ev[k] ) (void)hipEventDestroy( b->ctrl_ev[k] );
  (void)hipFree( b->d_ctrl ); if( b->h_ctrl ) (void)hipHostFree( b->h_ctrl );
  (void)hipFree( b->d_par ); for( int k=0; k<RKFD_PAR_COUNT; k++ ) free( b->h_par[k] );
  rkfd_links_destroy( b->links );
  rkfd_jac_destroy( b->jac );
  rkfd_dyn_destroy( b->dyn );
  rkfd_cf_destroy( b->cf );
  rkfd_reset_destroy( b->reset );
  if( b->spec_mod ) (void)hipModuleUnload( b->spec_mod );
  (void)hipFree( b->d_err ); (void)hipFree( b->dblob ); (void)hipFree( b->dblob2 );
  rkfd_devmodel_free( &b->host ); rkfd_devmodel_free( &b->host2 );
  free( b );
}

/* host-only: LDS bytes one instance of world m would occupy (no GPU needed) */
extern "C" int rkfdLdsBytesFor(const rkfdModel *m, int max_rigid)
{
  rkfdDevModelHost h;
  char err[256];
  if( !m || rkfd_devmodel_build( m, max_rigid, &h, err, sizeof(err) ) < 0 ){ SETERR( "rkfdLdsBytesFor: %s", m ? err : "null model" ); return -1; }
  const int n = (int)h.lds_bytes;
  rkfd_devmodel_free( &h );
  return n;
}

/* what a workgroup of the kernel with two instances per wavefront asks for: two instance blocks (and the diagnostic pad) */
static size_t wg2_bytes(const rkfdBatch *b){ return 2*b->host2.lds_bytes + b->lds_pad; }

extern "C" int rkfdBatchSize(const rkfdBatch *b){ return b ? b->batch : -1; }
extern "C" int rkfdBatchDof(const rkfdBatch *b){ return b ? b->ndof : -1; }
extern "C" int rkfdBatchLdsBytes(const rkfdBatch *b){ return b ? (int)b->lds_bytes : -1; }
extern "C" int rkfdBatchResidency(const rkfdBatch *b)
{
  int n = 0;
  if( !b ) return -1;
  if( hipOccupancyMaxActiveBlocksPerMultiprocessor( &n, (const void *)b->kern, RKFD_WAVE, b->lds_bytes ) != hipSuccess ) return -1;
  /* the runtime's answer is optimistic about LDS: the hardware hands it out in 1280-byte pieces, 128 per CU
   * (measured with tools/ubench/residency.hip, profiles/r01_lds_residency.txt), e.g. 16160 bytes -> 9, not 10 */
  const int pieces = (int)( ( b->lds_bytes + 1279 )/1280 );
  if( pieces > 0 && 128/pieces < n ) n = 128/pieces;
  if( b->ipw == 2 && b->spec_fn ){
    /* two instances per wavefront: workgroups of 2 x the LDS, at most two waves per SIMD (the kernel is built for that) */
    const int p2 = (int)( ( wg2_bytes( b ) + 1279 )/1280 );
    int w = p2 > 0 ? 128/p2 : 0;
    if( w > 8 ) w = 8;
    n = 2*w;
  }
  return n;
}
extern "C" double *rkfdBatchDevDis(rkfdBatch *b){ return b ? b->st.dis : NULL; }
extern "C" double *rkfdBatchDevVel(rkfdBatch *b){ return b ? b->st.vel : NULL; }
extern "C" double *rkfdBatchDevAcc(rkfdBatch *b){ return b ? b->st.acc : NULL; }

#define H2D(dst, src, bytes) do{ if( src ) HIPCHK( hipMemcpy( dst, src, bytes, hipMemcpyHostToDevice ), -1 ); }while(0)
#define D2H(dst, src, bytes) do{ if( dst ) HIPCHK( hipMemcpy( dst, src, bytes, hipMemcpyDeviceToHost ), -1 ); }while(0)

static int sync_streams(rkfdBatch *b);      /* the synchronous accessors wait for split launches first */

extern "C" int rkfdBatchSetState(rkfdBatch *b, const double *dis, const double *vel)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  const size_t n = sizeof(double)*(size_t)b->batch*b->ndof;
  H2D( b->st.dis, dis, n ); H2D( b->st.vel, vel, n );
  return 0;
}
extern "C" int rkfdBatchGetState(rkfdBatch *b, double *dis, double *vel, double *acc)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  const size_t n = sizeof(double)*(size_t)b->batch*b->ndof;
  D2H( dis, b->st.dis, n ); D2H( vel, b->st.vel, n ); D2H( acc, b->st.acc, n );
  return 0;
}
extern "C" int rkfdBatchSetMotorInput(rkfdBatch *b, const double *input)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  H2D( b->st.motor_in, input, sizeof(double)*(size_t)b->batch*b->nlink );
  return 0;
}
extern "C" int rkfdBatchGetContact(rkfdBatch *b, int *active, int *type, double *ref, double *f)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  const size_t n = (size_t)b->batch*b->ncand;
  std::vector<int> act( n );
  HIPCHK( hipMemcpy( act.data(), b->st.cv_active, sizeof(int)*n, hipMemcpyDeviceToHost ), -1 );
  D2H( type, b->st.cv_type, sizeof(int)*n );
  D2H( ref, b->st.cv_ref, sizeof(double)*3*n ); D2H( f, b->st.cv_f, sizeof(double)*3*n );
  /* a candidate out of contact has no state: the device keeps whatever it last held there
   * (it is rewritten at the next first contact), the boundary reports zeros */
  if( ref && n ) rkfd_ref_to_model( &b->host, ref, n );      /* device link frame -> model link frame */
  for( size_t i=0; i<n; i++ ){
    if( active ) active[i] = act[i];
    if( act[i] ) continue;
    if( type ) type[i] = 0;
    if( ref ) ref[3*i] = ref[3*i+1] = ref[3*i+2] = 0;
    if( f ) f[3*i] = f[3*i+1] = f[3*i+2] = 0;
  }
  return 0;
}
extern "C" int rkfdBatchSetContact(rkfdBatch *b, const int *active, const int *type, const double *ref)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  const size_t n = (size_t)b->batch*b->ncand;
  H2D( b->st.cv_active, active, sizeof(int)*n ); H2D( b->st.cv_type, type, sizeof(int)*n );
  if( ref && n ){
    std::vector<double> rd( ref, ref + 3*n );
    rkfd_ref_to_device( &b->host, rd.data(), n );             /* model link frame -> device link frame */
    HIPCHK( hipMemcpy( b->st.cv_ref, rd.data(), sizeof(double)*3*n, hipMemcpyHostToDevice ), -1 );
  }
  return 0;
}
extern "C" int rkfdBatchGetPivot(rkfdBatch *b, int *type, double *prev_trq)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  const size_t n = (size_t)b->batch*b->nlink;
  D2H( type, b->st.piv_type, sizeof(int)*n ); D2H( prev_trq, b->st.piv_prev, sizeof(double)*n );
  return 0;
}
/* breakable float joints: 1 per link whose joint has broken, [batch][nlink] */
extern "C" int rkfdBatchGetBroken(rkfdBatch *b, int *broken)
{
  if( !b || !broken ){ SETERR( "null argument" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  D2H( broken, b->st.brk, sizeof(int)*(size_t)b->batch*b->nlink );
  return 0;
}
extern "C" int rkfdBatchSetBroken(rkfdBatch *b, const int *broken)
{
  if( !b || !broken ){ SETERR( "null argument" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  H2D( b->st.brk, broken, sizeof(int)*(size_t)b->batch*b->nlink );
  return 0;
}
extern "C" int rkfdBatchSetPivot(rkfdBatch *b, const int *type, const double *prev_trq)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  const size_t n = (size_t)b->batch*b->nlink;
  H2D( b->st.piv_type, type, sizeof(int)*n ); H2D( b->st.piv_prev, prev_trq, sizeof(double)*n );
  return 0;
}

/* next start / stop pair of the timing pool (grown in blocks: creating events inside the launch path is expensive);
 * pairs are handed out whole, so a failed creation never leaves the pool misaligned */
static int timing_pair(rkfdBatch *b, hipEvent_t *e0, hipEvent_t *e1)
{
  *e0 = *e1 = NULL;
  if( b->tused + 2 > b->tev->size() ){
    for( int i=0; i<1024; i++ ){
      hipEvent_t a = NULL, c = NULL;
      if( hipEventCreate( &a ) != hipSuccess ) break;
      if( hipEventCreate( &c ) != hipSuccess ){ (void)hipEventDestroy( a ); break; }
      b->tev->push_back( a ); b->tev->push_back( c );
    }
    if( b->tused + 2 > b->tev->size() ) return 0;
  }
  *e0 = (*b->tev)[b->tused]; *e1 = (*b->tev)[b->tused+1];
  b->tused += 2;
  return 1;
}
/* make `stream` wait for everything the internal streams hold (no host synchronisation) */
static int join_streams(rkfdBatch *b, hipStream_t stream)
{
  if( b->nsplit > 1 && b->pending ){
    for( int k=0; k<b->nsplit; k++ ) HIPCHK( hipStreamWaitEvent( stream, b->done[k], 0 ), -1 );
    b->pending = 0;
  }
  return 0;
}
/* host waits for the internal streams and for the caller's stream of the batch's last launch (used by the synchronous accessors:
 * their blocking copies go over the null stream, which a stream made with hipStreamNonBlocking - the node level's, torch's - is not
 * ordered against).  Launches a caller spread over FURTHER streams of its own must be joined by the caller first. */
static int sync_streams(rkfdBatch *b)
{
  if( b->nsplit > 1 ) for( int k=0; k<b->nsplit; k++ ) HIPCHK( hipStreamSynchronize( b->sub[k] ), -1 );
  b->pending = 0;
  /* (the stream of the last launch must still exist here - include/rkfd_hip.h; once waited for, by this or by rkfdBatchStatus on
   *  it, it is not touched again until the next launch names one) */
  if( b->launched ){ HIPCHK( hipStreamSynchronize( b->last_stream ), -1 ); b->launched = 0; }
  return 0;
}
/* the device model a launch passes: with a table of per-instance parameters, the pointers to those parameters point at its first
 * row (the layout of rkfd_devmodel_par_row); both device models of a batch have the same device links */
static rkfdDevModel par_model(const rkfdBatch *b, const rkfdDevModel &dm)
{
  rkfdDevModel d = dm;
  if( b->d_par ) rkfd_devmodel_par_bind( &d, b->d_par );
  return d;
}
/* one kernel launch over `count` instances starting at `first`: the kernel compiled for this world when there is one */
/* ctrl / ctrl_stride: the control schedule of this launch's first step (NULL: the motor input in the state holds) */
static int launch_one(rkfdBatch *b, rkfdKernel kern, int count, int first, int mode, int nsteps, hipStream_t stream,
                      const double *ctrl = NULL, int ctrl_stride = 0)
{
  /* (a world-specific kernel always matches the batch: rkfdBatchSetParam / ClearParams rebuild it when the table comes or goes) */
  int pstride = b->d_par ? b->par_stride : 0;
  if( b->spec_fn && !b->st.prof ){
    rkfdDevModel dmp = par_model( b, b->ipw == 2 ? b->dm2 : b->dm );
    if( b->ipw == 2 ){
      /* two instances per wavefront: half as many workgroups, each with the LDS of two instances; the kernel learns where the
       * part ends through st.batch (a half beyond it is a stand-in that stores nothing) */
      rkfdDevState st2 = b->st;
      st2.batch = first + count;
      void *args[] = { &dmp, &st2, &first, &mode, &nsteps, &b->d_err, &ctrl, &ctrl_stride, &pstride };      /* (the ninth: kernels with a table only) */
      HIPCHK( hipModuleLaunchKernel( b->spec_fn, ( count+1 )/2, 1, 1, RKFD_WAVE, 1, 1, (unsigned)wg2_bytes( b ), stream, args, NULL ), -1 );
      return 0;
    }
    void *args[] = { &dmp, &b->st, &first, &mode, &nsteps, &b->d_err, &ctrl, &ctrl_stride, &pstride };
    HIPCHK( hipModuleLaunchKernel( b->spec_fn, count, 1, 1, RKFD_WAVE, 1, 1, (unsigned)b->lds_bytes, stream, args, NULL ), -1 );
    return 0;
  }
  if( b->d_par ){
    rkfdKernelPar kp = kern == b->kern_prof ? b->kern_prof_par : b->kern_par;
    hipLaunchKernelGGL( kp, dim3( count ), dim3( RKFD_WAVE ), b->lds_bytes, stream, par_model( b, b->dm ), b->st, first, mode, nsteps, b->d_err, ctrl, ctrl_stride, pstride );
  }
  else hipLaunchKernelGGL( kern, dim3( count ), dim3( RKFD_WAVE ), b->lds_bytes, stream, b->dm, b->st, first, mode, nsteps, b->d_err, ctrl, ctrl_stride );
  HIPCHK( hipGetLastError(), -1 );
  return 0;
}

/* the host schedule's block of instances [lo, hi) from the pinned staging into the device copy, on the stream that steps them;
 * ctrl_ev[ev] marks its end */
static int ctrl_upload(rkfdBatch *b, int lo, int hi, int nsteps, hipStream_t s, int ev)
{
  const size_t row = (size_t)nsteps*b->nlink, off = (size_t)lo*row;
  HIPCHK( hipMemcpyAsync( b->d_ctrl + off, b->h_ctrl + off, sizeof(double)*row*(size_t)( hi-lo ), hipMemcpyHostToDevice, s ), -1 );
  HIPCHK( hipEventRecord( b->ctrl_ev[ev], s ), -1 );
  if( ev + 1 > b->ctrl_nev ) b->ctrl_nev = ev + 1;
  return 0;
}
/* ctrl: NULL, or a control schedule [batch][nsteps][nlink] on the device (mode 0); upload: it is the batch's own copy, and every
 * part first brings its block over from the pinned staging (ctrl_upload) */
static int launch(rkfdBatch *b, int mode, int nsteps, void *stream, const double *ctrl = NULL, bool upload = false)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  rkfdKernel kern = b->st.prof ? b->kern_prof : b->kern;
  b->last_stream = (hipStream_t)stream; b->launched = 1;
  const int cstride = ctrl ? nsteps*b->nlink : 0;
  if( b->nsplit <= 1 || b->st.prof ){
    if( b->st.prof && sync_streams( b ) < 0 ) return -1;
    if( upload && ctrl_upload( b, 0, b->batch, nsteps, (hipStream_t)stream, 0 ) < 0 ) return -1;
    hipEvent_t e0 = NULL, e1 = NULL;
    if( b->timing && !b->st.prof && timing_pair( b, &e0, &e1 ) ) HIPCHK( hipEventRecord( e0, (hipStream_t)stream ), -1 );
    if( launch_one( b, kern, b->batch, 0, mode, nsteps, (hipStream_t)stream, ctrl, cstride ) < 0 ) return -1;
    if( e0 && e1 ) HIPCHK( hipEventRecord( e1, (hipStream_t)stream ), -1 );
    return 0;
  }
  /* fork: the parts start after what the caller's stream holds now; they do NOT wait for each other, and the
   * caller's stream does not wait for them until rkfdBatchJoin / rkfdBatchStatus */
  HIPCHK( hipEventRecord( b->fork, (hipStream_t)stream ), -1 );
  for( int k=0; k<b->nsplit; k++ ) HIPCHK( hipStreamWaitEvent( b->sub[k], b->fork, 0 ), -1 );
  /* several steps go out as that many rounds of one-step launches, not as fused kernels: a fused launch holds its
   * slots for all its steps, so with more instances than slots the rest of the batch waits that long and the tail
   * of the last round runs thin (4096 instances, 200 steps: 9.2 M steps/s fused, 12.7 M in rounds; tools/fused_vs_stepwise.py) */
  /* (not for worlds under the Vert plugin: the QP makes the step times of the instances vary widely, and there the
   * per-step barrier of a round costs more than the slots a fused launch holds: 2.1 M against 3.6 M steps/s) */
  /* (round 3: not one step per launch either - rounds of b->steps_per_launch steps, 5 by default: rollouts of 25 steps on config 4,
   *  steps per launch 1 / 2 / 3 / 5 / 9 / 13 / 25: 11.51 / 11.63 / 11.65 / 11.82 / 11.79 / 11.82 / 11.76 M steps/s - a launch loads
   *  an instance's state and the world's tables once, against slots held a little longer; profiles/r03_steps_per_launch.txt) */
  int rounds = 1, per = nsteps;
  if( mode == 0 && nsteps > 1 && !b->dm.vert_rigid ){ per = b->steps_per_launch < nsteps ? b->steps_per_launch : nsteps; rounds = ( nsteps + per - 1 )/per; }
  for( int r=0; r<rounds; r++ )
    for( int k=0; k<b->nsplit; k++ ){
      const int lo = (int)( (long long)b->batch*k/b->nsplit ), hi = (int)( (long long)b->batch*( k+1 )/b->nsplit );
      if( hi <= lo ) continue;
      /* (the part's block of the batch's copy is read by this part only: its upload waits for nothing but its own earlier steps) */
      if( upload && r == 0 && ctrl_upload( b, lo, hi, nsteps, b->sub[k], k ) < 0 ) return -1;
      hipEvent_t e0 = NULL, e1 = NULL;
      if( b->timing && timing_pair( b, &e0, &e1 ) ) HIPCHK( hipEventRecord( e0, b->sub[k] ), -1 );
      /* round r starts at step r per of the schedule; the stride of an instance stays that of the whole schedule */
      if( launch_one( b, kern, hi-lo, lo, mode, ( r+1 )*per <= nsteps ? per : nsteps - r*per, b->sub[k],
                      ctrl ? ctrl + (size_t)r*per*b->nlink : NULL, cstride ) < 0 ) return -1;
      if( e0 && e1 ) HIPCHK( hipEventRecord( e1, b->sub[k] ), -1 );
    }
  for( int k=0; k<b->nsplit; k++ ) HIPCHK( hipEventRecord( b->done[k], b->sub[k] ), -1 );
  b->pending = 1;
  return 0;
}
/* ---- the step kernel compiled for one world (hipRTC) ---------------------------------------------------- */
/* source of the specialised kernel: the dimensions of the world as literals in front of the same device code */
static std::string spec_source(const rkfdDevModel &d, int ipw = 1, int par = 0)
{
  char buf[4096];
  snprintf( buf, sizeof(buf),
    "#define RKFD_SPEC 1\n#define RKFD_W %d\n%s"
    "#define RKFD_SPEC_NLINK %d\n#define RKFD_SPEC_NDOF %d\n#define RKFD_SPEC_NCAND %d\n#define RKFD_SPEC_NLINK_MODEL %d\n"
    "#define RKFD_SPEC_NLEVEL %d\n#define RKFD_SPEC_NROUND %d\n#define RKFD_SPEC_NSCHED %d\n#define RKFD_SPEC_MAXRG %d\n"
    "#define RKFD_SPEC_NPOOL %d\n#define RKFD_SPEC_NFLOAT %d\n#define RKFD_SPEC_MAXACT %d\n#define RKFD_SPEC_NSIDE %d\n"
    "#define RKFD_SPEC_NPUROW %d\n#define RKFD_SPEC_PU_D0 %d\n#define RKFD_SPEC_PU_ALIAS %d\n#define RKFD_SPEC_VERT_RIGID %d\n#define RKFD_SPEC_QSCR_ALIAS %d\n"
    "#define RKFD_SPEC_HAS_SLIDE %d\n#define RKFD_SPEC_MA_SIZE %d\n#define RKFD_SPEC_MA_PACKED %d\n"
    "#define RKFD_SPEC_MAX_ITER %d\n#define RKFD_SPEC_SOLVER %d\n#define RKFD_SPEC_PYRAMID %d\n#define RKFD_SPEC_ANCHOR %d\n#define RKFD_SPEC_MLCP_MFMA %d\n"
    "#define RKFD_SPEC_HAS_BRF %d\n#define RKFD_SPEC_LDS_INSTANCE %d\n"
    "#define RKFD_SPEC_VOL_NPAIR %d\n#define RKFD_SPEC_VOL_NP %d\n#define RKFD_SPEC_VOL_NCP %d\n#define RKFD_SPEC_VOL_PV %d\n#define RKFD_SPEC_VOL_NF %d\n"
    "#include \"rkfd_device.h\"\n"
    "extern \"C\" __global__ void __launch_bounds__(64, %d)\n"
    "rkfd_step_kernel_spec(rkfdDevModel m, rkfdDevState st, int first, int mode, int nsteps, int *errflag, const double *ctrl, int ctrl_stride%s)\n"
    "{\n"
    "  extern __shared__ __attribute__((aligned(16))) char lds[];\n"
    "  int b = first + (int)blockIdx.x*RKFD_W + HALF();\n"
    "  if( RKFD_W == 1 && b >= st.batch ) return;\n"
    "  const bool live = b < st.batch;\n"
    "  if( !live ) b -= 1;\n"
    "  rkfd_instance<false, %s, %s>( m, st, b, lds + HALF()*RKFD_SPEC_LDS_INSTANCE, mode, nsteps, errflag, live, nullptr, ctrl, ctrl_stride%s );\n"
    "}\n",
    ipw, par ? "#define RKFD_PARAMS 1\n" : "", d.nlink, d.ndof, d.ncand, d.nlink_model, d.nlevel, d.nround, d.nsched, d.maxrg, d.npool, d.nfloat, d.maxact, d.nside,
    d.npurow, d.pu_d0, d.pu_alias, d.vert_rigid, d.qscr_alias, d.has_slide, d.ma_size, d.ma_packed, d.max_iter, d.solver, d.pyramid, d.anchor, d.mlcp_mfma,
    d.has_brf, d.lds_instance, d.vol_npair, d.vol_np, d.vol_ncp, d.vol_pv, d.vol_nf,
    ( d.vol_np > 0 || ipw == 2 || d.vert_rigid == 2 ) ? 2 : 3, par ? ", int par_stride" : "", d.vol_np > 0 ? "2" : ( d.vert_rigid ? "1" : "0" ), d.ma_packed ? "true" : "false",
    par ? ", par_stride" : "" );
  std::string src;
  if( const char *pre = getenv( "RKFD_SPEC_DEFINE" ) ){      /* diagnostic: NAME[,NAME...] defined as 1 in front of the source */
    std::string names( pre ); size_t p0 = 0;
    while( p0 < names.size() ){ size_t p1 = names.find( ',', p0 ); if( p1 == std::string::npos ) p1 = names.size(); src += "#define " + names.substr( p0, p1-p0 ) + " 1\n"; p0 = p1+1; }
  }
  return src + std::string( buf );
}
/* hipRTC, bound at run time in a PRIVATE link namespace.  hipRTC finds its compiler (libamd_comgr) by soname, and
 * a process serves every request for a soname with the first library it loaded under it: a host program that has
 * loaded a framework bundling an older comgr (PyTorch does) would silently get that compiler - with it this kernel
 * spills (437 VGPR spills, 3.9 M instead of 14 M steps/s on the humanoid).  dlmopen( LM_ID_NEWLM ) gives hipRTC and
 * the comgr next to it (RUNPATH $ORIGIN) a namespace of their own, whatever the host program loaded before or
 * after - no preload needed from a C, Python or any other caller.  The ROCm library directory is the one this
 * library was built against (RKFD_ROCM_LIBDIR, from the Makefile) unless RKFD_ROCM_LIBDIR / ROCM_PATH say otherwise;
 * RKFD_RTC_NAMESPACE=shared skips the private namespace (diagnostic). */
#ifndef RKFD_ROCM_LIBDIR
#define RKFD_ROCM_LIBDIR "/opt/rocm/lib"
#endif
struct rkfdRtc {
  void *h;
  int priv;     /* 1: loaded in a private namespace */
  hiprtcResult (*create)(hiprtcProgram *, const char *, const char *, int, const char **, const char **);
  hiprtcResult (*compile)(hiprtcProgram, int, const char **);
  hiprtcResult (*logsize)(hiprtcProgram, size_t *);
  hiprtcResult (*log)(hiprtcProgram, char *);
  hiprtcResult (*codesize)(hiprtcProgram, size_t *);
  hiprtcResult (*code)(hiprtcProgram, char *);
  hiprtcResult (*destroy)(hiprtcProgram *);
  const char *(*errstr)(hiprtcResult);
};
static const rkfdRtc *rtc_api(void)
{
  static rkfdRtc api;
  static int state = 0;          /* 0 not tried, 1 ready, -1 failed */
  static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
  pthread_mutex_lock( &mu );
  if( state == 0 ){
    std::string dir = RKFD_ROCM_LIBDIR;
    if( const char *e = getenv( "RKFD_ROCM_LIBDIR" ) ) dir = e;
    else if( const char *r = getenv( "ROCM_PATH" ) ){ std::string d = std::string( r ) + "/lib"; if( access( ( d + "/libhiprtc.so" ).c_str(), R_OK ) == 0 ) dir = d; }
    const char *mode = getenv( "RKFD_RTC_NAMESPACE" );
    const char *names[] = { "/libhiprtc.so.7", "/libhiprtc.so" };
    void *h = NULL; int priv = 0;
    if( !mode || strcmp( mode, "shared" ) != 0 )
      for( int k=0; k<2 && !h; k++ ) h = dlmopen( LM_ID_NEWLM, ( dir + names[k] ).c_str(), RTLD_NOW | RTLD_LOCAL );
    if( h ) priv = 1;
    for( int k=0; k<2 && !h; k++ ) h = dlopen( ( dir + names[k] ).c_str(), RTLD_NOW | RTLD_LOCAL );
    if( !h ) h = dlopen( "libhiprtc.so", RTLD_NOW | RTLD_LOCAL );
    if( !h ){ SETERR( "hipRTC: cannot load libhiprtc from %s: %s", dir.c_str(), dlerror() ); state = -1; }
    else {
      api.h = h; api.priv = priv;
#define RTCSYM(field, name) *(void **)&api.field = dlsym( h, name )
      RTCSYM( create, "hiprtcCreateProgram" ); RTCSYM( compile, "hiprtcCompileProgram" ); RTCSYM( logsize, "hiprtcGetProgramLogSize" );
      RTCSYM( log, "hiprtcGetProgramLog" ); RTCSYM( codesize, "hiprtcGetCodeSize" ); RTCSYM( code, "hiprtcGetCode" );
      RTCSYM( destroy, "hiprtcDestroyProgram" ); RTCSYM( errstr, "hiprtcGetErrorString" );
#undef RTCSYM
      if( !api.create || !api.compile || !api.logsize || !api.log || !api.codesize || !api.code || !api.destroy || !api.errstr ){
        SETERR( "hipRTC: %s lacks an entry point", dir.c_str() ); state = -1;
      } else state = 1;
    }
  }
  const int s = state;
  pthread_mutex_unlock( &mu );
  return s == 1 ? &api : NULL;
}
/* ---- ahead-of-time specialised kernels ---------------------------------------------------------------------
 * The world-specific kernel is a pure function of (the generated preamble, the device sources the library carries, the compiler
 * options): its code object can be made when the library is built and merely LOADED at run time.  `make spec` does that for the
 * worlds of BASELINE.json's configurations (tools/make_spec.py -> roki-fd_amd/spec/rkfd_spec_<key>.co, beside the library), so the
 * headline needs no run-time compiler; any other world is compiled through hipRTC on first use and - when the directory is
 * writable - kept there too.  The key is a 64-bit FNV-1a hash over preamble, sources and options: a stale file cannot be picked
 * up after the device code changed.  RKFD_SPEC_DIR names another directory; RKFD_SPEC_STORE=0 switches the store off. */
static unsigned long long spec_key(const std::string &src, const char *const *opts, int nopts)
{
  unsigned long long h = 1469598103934665603ull;
  auto eat = [&h](const char *p){ for( ; *p; p++ ){ h ^= (unsigned char)*p; h *= 1099511628211ull; } h ^= 0xffu; h *= 1099511628211ull; };
  eat( src.c_str() );
  for( int i=0; i<rkfd_src_count; i++ ){ eat( rkfd_src_name[i] ); eat( rkfd_src_text[i] ); }
  for( int i=0; i<nopts; i++ ) eat( opts[i] );
  return h;
}
static std::string spec_dir(void)
{
  if( const char *e = getenv( "RKFD_SPEC_DIR" ) ) return e;
  Dl_info di;
  if( dladdr( (const void *)&spec_key, &di ) && di.dli_fname ){
    std::string p( di.dli_fname );
    const size_t k = p.rfind( '/' );
    return ( k == std::string::npos ? std::string( "." ) : p.substr( 0, k ) ) + "/spec";
  }
  return "spec";
}
static bool spec_store_on(void){ const char *e = getenv( "RKFD_SPEC_STORE" ); return !( e && atoi( e ) == 0 ); }
static std::string spec_path(unsigned long long key)
{
  char nm[64];
  snprintf( nm, sizeof(nm), "/rkfd_spec_%016llx.co", key );
  return spec_dir() + nm;
}
static int spec_from_store(unsigned long long key, std::vector<char> &code)
{
  if( !spec_store_on() ) return -1;
  FILE *f = fopen( spec_path( key ).c_str(), "rb" );
  if( !f ) return -1;
  fseek( f, 0, SEEK_END ); const long n = ftell( f ); fseek( f, 0, SEEK_SET );
  int r = -1;
  if( n > 0 ){ code.resize( (size_t)n ); if( fread( code.data(), 1, (size_t)n, f ) == (size_t)n ) r = 0; }
  fclose( f );
  if( r == 0 && getenv( "RKFD_SPEC_DEBUG" ) ) fprintf( stderr, "rkfd: specialised kernel loaded from %s (no run-time compile)\n", spec_path( key ).c_str() );
  return r;
}
static void spec_to_store(unsigned long long key, const std::vector<char> &code)
{
  if( !spec_store_on() ) return;
  char uniq[48];
  snprintf( uniq, sizeof(uniq), ".tmp.%ld.%p", (long)getpid(), (void *)&code );      /* (several ranks of a node may compile the same world at once) */
  const std::string dir = spec_dir(), path = spec_path( key ), tmp = path + uniq;
  (void)mkdir( dir.c_str(), 0777 );
  FILE *f = fopen( tmp.c_str(), "wb" );
  if( !f ) return;                                  /* (a read-only installation: compile every time) */
  const bool ok = fwrite( code.data(), 1, code.size(), f ) == code.size();
  fclose( f );
  if( ok ) (void)rename( tmp.c_str(), path.c_str() ); else (void)remove( tmp.c_str() );
}
static int g_spec_last_from_store = 0;      /* diagnostic: did the last spec_compile of this thread's process hit the store */
extern "C" int rkfdSpecializeLastFromStore(void){ return g_spec_last_from_store; }

/* compile for gfx950 from the sources the library carries (rkfd_device_src.inc): nothing is read from disk but the store above */
static int spec_compile(const rkfdDevModel &d, std::vector<char> &code, int ipw = 1, int par = 0)
{
  const std::string src = spec_source( d, ipw, par );
  const char *opts[] = { "--offload-arch=gfx950", "-O3", "-Wno-unused-value", "-mllvm", "-disable-machine-licm" };
  const int nopts = (int)( sizeof(opts)/sizeof(opts[0]) );
  const unsigned long long key = spec_key( src, opts, nopts );
  g_spec_last_from_store = 0;
  if( !getenv( "RKFD_SPEC_DUMP" ) && spec_from_store( key, code ) == 0 ){
    g_spec_last_from_store = 1;
    if( const char *dump = getenv( "RKFD_SPEC_DUMP_CODE" ) ){ FILE *f = fopen( dump, "wb" ); if( f ){ fwrite( code.data(), 1, code.size(), f ); fclose( f ); } }
    return 0;
  }
  const rkfdRtc *rtc = rtc_api();
  if( !rtc ) return -1;
  /* one compile at a time: the environment snapshot below is per namespace, not per call */
  static pthread_mutex_t cmu = PTHREAD_MUTEX_INITIALIZER;
  struct Unlock { pthread_mutex_t *m; ~Unlock(){ pthread_mutex_unlock( m ); } } unlock = { &cmu };
  pthread_mutex_lock( &cmu );
  if( rtc->priv ){
    /* The private namespace carries its own copy of the C library, and that copy's `environ` still points at the array the
     * process had when the namespace was made.  The host's setenv (Python's os.environ, say) moves the real array and frees
     * the old one: the compiler's getenv would walk freed memory (seen: a segmentation fault in the 88th test of a pytest
     * process that had set new variables between two specialisations).  Round 2 pointed the copy at the host's live array
     * before every compile - which the host can move again DURING the compile (another thread's setenv), and which helper
     * threads or exit handlers of the namespace may still read after it.  Now the namespace gets an environment
     * of its OWN: a deep copy (array and strings) taken under this mutex before every compile, which nothing but this
     * function ever replaces.  Earlier snapshots are kept alive as long as the library is loaded (a thread of the namespace
     * may still hold a pointer into one): a few kilobytes per compile, one compile per world. */
    char ***penv = (char ***)dlsym( rtc->h, "environ" );
    if( penv && penv != &environ ){
      size_t n = 0, bytes = 0;
      for( char **e = environ; e && *e; e++ ){ n++; bytes += strlen( *e ) + 1; }
      char **arr = (char **)malloc( sizeof(char *)*( n+1 ) + bytes );
      if( arr ){
        char *p = (char *)( arr + n + 1 );
        size_t k = 0;
        for( char **e = environ; e && *e && k < n; e++, k++ ){ const size_t l = strlen( *e ) + 1; memcpy( p, *e, l ); arr[k] = p; p += l; }
        arr[k] = NULL;
        if( getenv( "RKFD_SPEC_DEBUG" ) ) fprintf( stderr, "rkfd: hipRTC's namespace gets its own snapshot of the environment (%zu variables)\n", k );
        *penv = arr;      /* (the previous snapshot is deliberately not freed, see above) */
      }
    }
  }
  if( const char *dump = getenv( "RKFD_SPEC_DUMP" ) ){ FILE *f = fopen( dump, "w" ); if( f ){ fputs( src.c_str(), f ); fclose( f ); } }   /* diagnostic */
  hiprtcProgram prog;
  if( rtc->create( &prog, src.c_str(), "rkfd_step_kernel_spec.hip", rkfd_src_count, (const char **)rkfd_src_text, (const char **)rkfd_src_name ) != HIPRTC_SUCCESS ){ SETERR( "hiprtcCreateProgram failed" ); return -1; }
  const hiprtcResult r = rtc->compile( prog, nopts, opts );
  if( r != HIPRTC_SUCCESS ){
    size_t n = 0; rtc->logsize( prog, &n );
    std::string log( n ? n : 1, ' ' ); if( n ) rtc->log( prog, &log[0] );
    SETERR( "hipRTC: %s: %.400s", rtc->errstr( r ), log.c_str() );
    rtc->destroy( &prog );
    return -1;
  }
  size_t n = 0;
  rtc->codesize( prog, &n ); code.resize( n ); rtc->code( prog, code.data() );
  if( const char *dump = getenv( "RKFD_SPEC_DUMP_CODE" ) ){ FILE *f = fopen( dump, "wb" ); if( f ){ fwrite( code.data(), 1, n, f ); fclose( f ); } }   /* diagnostic */
  rtc->destroy( &prog );
  if( rtc->priv ) spec_to_store( key, code );      /* (only what the compiler this library was built with produced: the private namespace) */
  return 0;
}
extern "C" int rkfdSpecializeCompileP(const rkfdModel *m, int max_rigid, int ipw, int par)
{
  rkfdDevModelHost h;
  char err[256];
  if( ipw != 1 && ipw != 2 ){ SETERR( "rkfdSpecializeCompileW: 1 or 2 instances per wavefront" ); return -1; }
  if( !m || rkfd_devmodel_build_w( m, max_rigid, ipw == 2 ? 4 : 8, &h, err, sizeof(err) ) < 0 ){ SETERR( "rkfdSpecializeCompile: %s", m ? err : "null model" ); return -1; }
  std::vector<char> code;
  const int r = spec_compile( h.dm, code, ipw, par ? 1 : 0 );
  rkfd_devmodel_free( &h );
  return r < 0 ? -1 : (int)code.size();
}
extern "C" int rkfdSpecializeCompileW(const rkfdModel *m, int max_rigid, int ipw){ return rkfdSpecializeCompileP( m, max_rigid, ipw, 0 ); }
extern "C" int rkfdSpecializeCompile(const rkfdModel *m, int max_rigid){ return rkfdSpecializeCompileW( m, max_rigid, 1 ); }
/* the world-specific kernel of the batch as it is set up (instances per wavefront), without (par = 0) or with a table of
 * per-instance parameters: compiled or taken from the store, loaded, checked - the batch itself is not touched */
static int spec_build(rkfdBatch *b, int par, hipModule_t *mod, hipFunction_t *fn)
{
  *mod = NULL; *fn = NULL;
  if( b->lds_bytes > 64*1024 ){ SETERR( "rkfdBatchSpecialize: worlds above 64 KiB of LDS per instance keep the generic kernel" ); return -1; }
  std::vector<char> code;
  if( spec_compile( b->ipw == 2 ? b->host2.dm : b->dm, code, b->ipw == 2 ? 2 : 1, par ) < 0 ) return -1;
  HIPCHK( hipModuleLoadData( mod, code.data() ), -1 );
  if( hipModuleGetFunction( fn, *mod, "rkfd_step_kernel_spec" ) != hipSuccess ){
    (void)hipModuleUnload( *mod ); *mod = NULL; *fn = NULL;
    SETERR( "rkfdBatchSpecialize: the code object lacks rkfd_step_kernel_spec" ); return -1;
  }
  if( b->ipw == 2 && wg2_bytes( b ) > 64*1024 ){
    /* (a workgroup of two instances above 64 KiB of LDS needs the opt-in, as the generic kernels get it in rkfdBatchCreate) */
    const hipError_t e = hipFuncSetAttribute( (const void *)*fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wg2_bytes( b ) );
    if( e != hipSuccess ){
      (void)hipModuleUnload( *mod ); *mod = NULL; *fn = NULL;
      SETERR( "hipFuncSetAttribute(LDS=%zu) failed: %s", wg2_bytes( b ), hipGetErrorString( e ) );
      return -1;
    }
  }
  {
    /* the compiler behind hipRTC is whichever libamd_comgr the process loaded first; a framework that bundles an older
     * one (PyTorch does) gives a kernel that spills (437 VGPR spills, 3.9 M instead of 14 M steps/s on config 4): refuse it */
    int regs = -1, scratch = -1;
    hipFuncGetAttribute( &regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, *fn );
    hipFuncGetAttribute( &scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, *fn );
    if( getenv( "RKFD_SPEC_DEBUG" ) ) fprintf( stderr, "rkfdBatchSpecialize: %d instance(s) per wavefront, %s table of per-instance parameters, %d VGPRs, %d bytes of scratch per lane, %zu bytes of LDS per instance\n", b->ipw == 2 ? 2 : 1, par ? "with a" : "no", regs, scratch, b->ipw == 2 ? b->host2.lds_bytes : b->lds_bytes );
    if( scratch > ( b->dm.vol_np > 0 ? 512 : 160 ) ){      /* (the Volume variant is built for two waves per SIMD and spills a few registers on purpose; worlds with two moving
                                                             * contact sides sit at the 168-register limit and spill a handful - tools/spec_resources.py; the wrong compiler: 912 B) */
      (void)hipModuleUnload( *mod ); *mod = NULL; *fn = NULL;
      SETERR( "rkfdBatchSpecialize: the compiler hipRTC resolved to in this process produced a spilling kernel (%d VGPRs, %d bytes of scratch per lane); "
              "point RKFD_ROCM_LIBDIR at the ROCm libraries this library was built with; the generic kernel stays in use", regs, scratch );
      return -1;
    }
  }
  return 0;
}
extern "C" int rkfdBatchSpecialize(rkfdBatch *b)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  if( b->spec_fn ) return 0;
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  hipModule_t mod; hipFunction_t fn;
  if( spec_build( b, b->d_par ? 1 : 0, &mod, &fn ) < 0 ) return -1;
  b->spec_mod = mod; b->spec_fn = fn; b->spec_par = b->d_par ? 1 : 0;
  return 0;
}

/* Two instances per wavefront (RKFD_W = 2, rkfd_devmodel.h): takes effect in the world-specific kernel - call before
 * rkfdBatchSpecialize.  Builds the second device model (sweep schedule with four links per iteration); fails with a message
 * when the world does not fit 32 lanes per instance. */
extern "C" int rkfdBatchSetInstancesPerWave(rkfdBatch *b, int ipw)
{
  if( !b || ( ipw != 1 && ipw != 2 ) ){ SETERR( "rkfdBatchSetInstancesPerWave: 1 or 2" ); return -1; }
  if( b->spec_fn ){ SETERR( "rkfdBatchSetInstancesPerWave: call it before rkfdBatchSpecialize" ); return -1; }
  if( ipw == 1 ){ b->ipw = 1; return 0; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( !b->dblob2 ){
    char err[256];
    if( rkfd_devmodel_build_w( b->model_for_w2, b->host.dm.maxrg, 4, &b->host2, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchSetInstancesPerWave: %s", err ); return -1; }
    if( wg2_bytes( b ) > 160*1024 ){ SETERR( "rkfdBatchSetInstancesPerWave: two instances need %zu bytes of LDS (> 160 KiB)", wg2_bytes( b ) ); rkfd_devmodel_free( &b->host2 ); return -1; }
    HIPCHK( hipMalloc( &b->dblob2, b->host2.bytes ), -1 );
    HIPCHK( hipMemcpy( b->dblob2, b->host2.blob, b->host2.bytes, hipMemcpyHostToDevice ), -1 );
    b->dm2 = b->host2.dm;
    rkfd_devmodel_rebase( &b->dm2, b->host2.blob, b->dblob2 );
  }
  b->ipw = 2;
  return 0;
}
extern "C" int rkfdBatchInstancesPerWave(const rkfdBatch *b){ return b ? ( b->ipw == 2 && b->spec_fn ? 2 : 1 ) : -1; }


/* rkfdBatchTuneInstancesPerWave: MEASURE which of the two mappings is faster for this world on this device at this batch
 * size, and keep it.  The two give the same results to the last bit (tests/test_gpu_edge.py: two_instances_per_wavefront), so
 * the choice changes the time of a step and nothing else.  The batch must hold a state to step from (rkfdBatchSetState +
 * rkfdBatchUpdateInit); the state is put back as it was, an earlier rkfdBatchSnapshot is left alone.  Compiles both kernels
 * (or takes them from the ahead-of-time store).  Returns the chosen count (1 or 2), -1 on error; ms[2] (may be NULL) gets
 * the milliseconds of nsteps steps under either (ms[1] < 0: the world is not eligible for two - rkfdLastError says why).
 * Which wins is a property of the world: two instances per wavefront halve the instructions issued per step, but not the
 * LDS an instance holds, so they win where the step is bound by instruction issue (config 1b, 2, 3: +20 %, +16 %, +5 %) and
 * lose where it is bound by how many instances the LDS lets a CU hold (config 4: -4 %); profiles/r03_ipw_ab.txt. */
static int tune_time(rkfdBatch *b, int nsteps, double *ms)
{
  hipEvent_t e0, e1;
  HIPCHK( hipEventCreate( &e0 ), -1 ); HIPCHK( hipEventCreate( &e1 ), -1 );
  int r = 0;
  float best = -1;
  for( int rep=0; rep<3 && r == 0; rep++ ){      /* first pass: warm-up (code object upload, clocks); then the faster of two */
    if( rkfdBatchRestore( b, NULL ) < 0 || rkfdBatchJoin( b, NULL ) < 0 ){ r = -1; break; }
    if( hipEventRecord( e0, NULL ) != hipSuccess || rkfdBatchUpdate( b, nsteps, NULL ) < 0 || rkfdBatchJoin( b, NULL ) < 0
        || hipEventRecord( e1, NULL ) != hipSuccess || hipEventSynchronize( e1 ) != hipSuccess ){ r = -1; break; }
    float t = 0;
    (void)hipEventElapsedTime( &t, e0, e1 );
    if( rep > 0 && ( best < 0 || t < best ) ) best = t;
  }
  (void)hipEventDestroy( e0 ); (void)hipEventDestroy( e1 );
  *ms = best;
  return r;
}
extern "C" int rkfdBatchTuneInstancesPerWave(rkfdBatch *b, int nsteps, double *ms)
{
  if( !b || nsteps < 1 ){ SETERR( "rkfdBatchTuneInstancesPerWave: bad arguments" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  double t[2] = { -1, -1 };
  if( ms ){ ms[0] = ms[1] = -1; }
  /* the caller's snapshot steps aside for the one the measurement restores from */
  const rkfdDevState keep = b->snap;
  const int had = b->has_snap;
  b->has_snap = 0; memset( &b->snap, 0, sizeof(b->snap) );
  int r = rkfdBatchSnapshot( b );
  int chosen = -1;
  if( r == 0 ){
    /* (a) what the batch has now, brought to one instance per wavefront */
    if( b->spec_fn && b->ipw == 2 ){ (void)hipModuleUnload( b->spec_mod ); b->spec_mod = NULL; b->spec_fn = NULL; }
    b->ipw = 1;
    r = rkfdBatchSpecialize( b );
    if( r == 0 ) r = tune_time( b, nsteps, &t[0] );
  }
  if( r == 0 ){
    /* (b) two: set the first kernel aside, build the second */
    hipModule_t mod1 = b->spec_mod; hipFunction_t fn1 = b->spec_fn;
    b->spec_mod = NULL; b->spec_fn = NULL;
    int two = rkfdBatchSetInstancesPerWave( b, 2 );
    if( two == 0 ) two = rkfdBatchSpecialize( b );
    /* a failed measurement of two (a launch the device refuses, say) makes the world not eligible, as a failed build does:
     * one instance per wavefront stays, and t[1] < 0 says so; the state goes back from the snapshot below either way */
    if( two == 0 && tune_time( b, nsteps, &t[1] ) < 0 ){ two = -1; t[1] = -1; (void)hipGetLastError(); }
    if( two == 0 && t[1] < t[0] ){ (void)hipModuleUnload( mod1 ); chosen = 2; }
    else{
      if( b->spec_mod ) (void)hipModuleUnload( b->spec_mod );
      b->spec_mod = mod1; b->spec_fn = fn1; b->ipw = 1;
      chosen = 1;
    }
  }
  /* the state as it was, and the caller's snapshot back in place */
  if( b->has_snap ){
    if( rkfdBatchRestore( b, NULL ) < 0 || rkfdBatchJoin( b, NULL ) < 0 || hipDeviceSynchronize() != hipSuccess ) chosen = -1;
    (void)hipFree( b->snap.dis ); (void)hipFree( b->snap.vel ); (void)hipFree( b->snap.acc );
    (void)hipFree( b->snap.piv_type ); (void)hipFree( b->snap.piv_prev ); (void)hipFree( b->snap.brk );
    (void)hipFree( b->snap.cv_active ); (void)hipFree( b->snap.cv_type ); (void)hipFree( b->snap.cv_ref ); (void)hipFree( b->snap.cv_f );
  }
  b->snap = keep; b->has_snap = had;
  if( ms ){ ms[0] = t[0]; ms[1] = t[1]; }
  return chosen;
}

extern "C" int rkfdBatchSetStepsPerLaunch(rkfdBatch *b, int n)
{
  if( !b || n < 1 ){ SETERR( "rkfdBatchSetStepsPerLaunch: n >= 1" ); return -1; }
  b->steps_per_launch = n;
  return 0;
}
extern "C" int rkfdBatchSetSplit(rkfdBatch *b, int nsplit)
{
  if( !b || nsplit < 1 || nsplit > RKFD_MAX_SPLIT ){ SETERR( "rkfdBatchSetSplit: 1 <= nsplit <= %d", RKFD_MAX_SPLIT ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  if( nsplit > 1 && !b->fork ){
    HIPCHK( hipEventCreateWithFlags( &b->fork, hipEventDisableTiming ), -1 );
    for( int k=0; k<RKFD_MAX_SPLIT; k++ ){
      HIPCHK( hipStreamCreateWithFlags( &b->sub[k], hipStreamNonBlocking ), -1 );
      HIPCHK( hipEventCreateWithFlags( &b->done[k], hipEventDisableTiming ), -1 );
    }
  }
  b->nsplit = nsplit;
  return 0;
}
extern "C" int rkfdBatchJoin(rkfdBatch *b, void *stream)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  return join_streams( b, (hipStream_t)stream );
}
extern "C" int rkfdBatchTimeLaunches(rkfdBatch *b, int on)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  b->tused = 0;
  b->timing = on ? 1 : 0;
  if( on && b->tev->empty() ){ hipEvent_t e0, e1; (void)timing_pair( b, &e0, &e1 ); b->tused = 0; }     /* pre-create the first block */
  return 0;
}
extern "C" int rkfdBatchLaunchTiming(rkfdBatch *b, int *launches, double *total_ms)
{
  if( !b || !launches || !total_ms ){ SETERR( "rkfdBatchLaunchTiming: bad arguments" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  HIPCHK( hipDeviceSynchronize(), -1 );
  *launches = (int)( b->tused/2 ); *total_ms = 0;
  for( size_t i=0; i+1<b->tused; i+=2 ){
    float ms = 0;
    HIPCHK( hipEventElapsedTime( &ms, (*b->tev)[i], (*b->tev)[i+1] ), -1 );
    *total_ms += ms;
  }
  return 0;
}
extern "C" int rkfdBatchUpdateInit(rkfdBatch *b, void *stream){ return launch( b, 1, 0, stream ); }
extern "C" int rkfdBatchUpdate(rkfdBatch *b, int nsteps, void *stream)
{
  if( nsteps < 1 ){ SETERR( "rkfdBatchUpdate: nsteps must be >= 1" ); return -1; }
  return launch( b, 0, nsteps, stream );
}
extern "C" int rkfdBatchEval(rkfdBatch *b, int doUpRef, void *stream){ return launch( b, doUpRef ? 1 : 2, 0, stream ); }

/* nsteps x ( rkJointMotorSetInput; rkFDUpdate ) with the inputs of a control schedule u[batch][nsteps][nlink]: the same bits as
 * nsteps x ( rkfdBatchSetMotorInput( u[:, k, :] ); rkfdBatchUpdate( 1 ) ), in the launches rkfdBatchUpdate makes (split parts,
 * steps per launch, the world-specific kernel).  Host schedule: copied into pinned staging before the call returns, then to the
 * batch's device copy in stream order. */
extern "C" int rkfdBatchUpdateControlled(rkfdBatch *b, int nsteps, const double *u, void *stream)
{
  if( !b || !u || nsteps < 1 ){ SETERR( "rkfdBatchUpdateControlled: %s", !b ? "null batch" : !u ? "null schedule" : "nsteps must be >= 1" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  const size_t n = (size_t)b->batch*nsteps*b->nlink;
  /* the staging may still feed the copies of the previous call (they wait for its steps on the streams that made them) */
  for( int k=0; k<b->ctrl_nev; k++ ) HIPCHK( hipEventSynchronize( b->ctrl_ev[k] ), -1 );
  if( n > b->ctrl_cap ){
    /* the old device copy may still be read by launches of earlier calls */
    if( sync_streams( b ) < 0 ) return -1;
    HIPCHK( hipDeviceSynchronize(), -1 );
    (void)hipFree( b->d_ctrl ); b->d_ctrl = NULL;
    if( b->h_ctrl ){ (void)hipHostFree( b->h_ctrl ); b->h_ctrl = NULL; }
    b->ctrl_cap = 0;
    HIPCHK( hipMalloc( (void **)&b->d_ctrl, sizeof(double)*n ), -1 );
    HIPCHK( hipHostMalloc( (void **)&b->h_ctrl, sizeof(double)*n, hipHostMallocDefault ), -1 );
    b->ctrl_cap = n;
  }
  if( !b->ctrl_ev[0] )
    for( int k=0; k<RKFD_MAX_SPLIT; k++ ) HIPCHK( hipEventCreateWithFlags( &b->ctrl_ev[k], hipEventDisableTiming ), -1 );
  memcpy( b->h_ctrl, u, sizeof(double)*n );
  return launch( b, 0, nsteps, stream, b->d_ctrl, true );
}
/* the same with a schedule the caller keeps on the batch's device ([batch][nsteps][nlink] doubles), read in stream order after
 * `stream`: it must stay untouched until the steps are done (rkfdBatchJoin / rkfdBatchStatus) */
extern "C" int rkfdBatchUpdateControlledDev(rkfdBatch *b, int nsteps, const double *u_dev, void *stream)
{
  if( !b || !u_dev || nsteps < 1 ){ SETERR( "rkfdBatchUpdateControlledDev: %s", !b ? "null batch" : !u_dev ? "null schedule" : "nsteps must be >= 1" ); return -1; }
  return launch( b, 0, nsteps, stream, u_dev, false );
}

/* ---- per-instance physical parameters ----------------------------------------------------------------------- */
static const double *model_par(const rkfdModel *m, int which)
{
  switch( which ){
  case RKFD_PAR_MASS: return m->mass; case RKFD_PAR_COM: return m->com; case RKFD_PAR_INERTIA: return m->inertia;
  case RKFD_PAR_STIFF: return m->stiff; case RKFD_PAR_VISC: return m->visc; case RKFD_PAR_COULOMB: return m->coulomb; case RKFD_PAR_SFRIC: return m->sfric;
  case RKFD_PAR_CI_SF: return m->ci_sf; case RKFD_PAR_CI_KF: return m->ci_kf; case RKFD_PAR_CI_K: return m->ci_k;
  case RKFD_PAR_CI_L: return m->ci_l; case RKFD_PAR_CI_E: return m->ci_e; case RKFD_PAR_CI_V: return m->ci_v;
  }
  return NULL;
}
static const char *const g_par_name[RKFD_PAR_COUNT] = { "mass", "com", "inertia", "stiff", "visc", "coulomb", "sfric", "ci_sf", "ci_kf", "ci_k", "ci_l", "ci_e", "ci_v" };
extern "C" int rkfdBatchParamWidth(const rkfdBatch *b, int which)
{
  if( !b || which < 0 || which >= RKFD_PAR_COUNT ) return -1;
  if( which >= RKFD_PAR_CI_SF ) return b->model_for_w2->nci;
  return b->nlink*( which == RKFD_PAR_COM ? 3 : ( which == RKFD_PAR_INERTIA ? 9 : 1 ) );
}
extern "C" int rkfdBatchHasParams(const rkfdBatch *b){ return b && b->d_par ? 1 : 0; }
/* what rkfdBatchSetParam refuses (nothing has been changed when it does) */
static int par_check(const rkfdBatch *b, int which, const double *values)
{
  if( !b ){ SETERR( "rkfdBatchSetParam: null batch" ); return -1; }
  if( which < 0 || which >= RKFD_PAR_COUNT ){ SETERR( "rkfdBatchSetParam: unknown parameter key %d (0 .. %d)", which, RKFD_PAR_COUNT-1 ); return -1; }
  if( !values ) return 0;
  const int w = rkfdBatchParamWidth( b, which );
  for( int i=0; i<b->batch; i++ )
    for( int j=0; j<w; j++ ){
      const double x = values[(size_t)i*w+j];
      if( !( x - x == 0.0 ) ){ SETERR( "rkfdBatchSetParam: %s of instance %d, entry %d is not finite", g_par_name[which], i, j ); return -1; }
      if( which == RKFD_PAR_MASS && x < 0 ){ SETERR( "rkfdBatchSetParam: negative mass %g for link %d of instance %d", x, j, i ); return -1; }
      if( which == RKFD_PAR_MASS && x == 0 && b->model_for_w2->mass[j] > 0 ){
        SETERR( "rkfdBatchSetParam: mass 0 for link %d of instance %d, whose mass is positive in the model (a massless link is another world)", j, i );
        return -1;
      }
    }
  return 0;
}
/* what the table's launches may still be reading: the internal streams and the caller's stream of the last launch (launches a
 * caller made on OTHER streams of its own must be joined by the caller first: rkfdBatchJoin / rkfdBatchStatus) */
static int par_quiesce(rkfdBatch *b){ return sync_streams( b ); }
/* the device table from a host copy h[key][batch][width]: every instance's row through rkfd_devmodel_par_row */
static int par_upload(rkfdBatch *b, double *const *h, double *d, size_t stride)
{
  std::vector<double> tab( (size_t)b->batch*stride + 1 );
  for( int i=0; i<b->batch; i++ ){
    const double *par[RKFD_PAR_COUNT];
    for( int k=0; k<RKFD_PAR_COUNT; k++ ) par[k] = h[k] + (size_t)i*rkfdBatchParamWidth( b, k );
    rkfd_devmodel_par_row( &b->host, par, &tab[(size_t)i*stride] );
  }
  HIPCHK( hipMemcpy( d, tab.data(), sizeof(double)*(size_t)b->batch*stride, hipMemcpyHostToDevice ), -1 );
  return 0;
}
/* Everything that can fail - the allocations, the world-specific kernel for batches with a table when the batch runs a
 * world-specific kernel (from the store `make spec` fills for the configurations of BASELINE.json, else a run-time compile of a few
 * seconds, kept in the store), the upload - happens BEFORE the batch is touched: a call that returns -1 has changed nothing. */
extern "C" int rkfdBatchSetParam(rkfdBatch *b, int which, const double *values)
{
  if( par_check( b, which, values ) < 0 ) return -1;
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( par_quiesce( b ) < 0 ) return -1;
  const int w = rkfdBatchParamWidth( b, which );
  if( b->d_par ){
    /* a table exists: the new values of this key into a copy of its array, the table rebuilt in place only once nothing can fail
     * but the copy to the device (which leaves the host copy as it was, and the next successful Set rewrites the whole table) */
    const size_t n = (size_t)b->batch*w;
    double *nk = (double *)malloc( sizeof(double)*( n + 1 ) );
    if( !nk ){ SETERR( "rkfdBatchSetParam: out of memory" ); return -1; }
    if( values ) memcpy( nk, values, sizeof(double)*n );
    else for( int i=0; i<b->batch; i++ ) memcpy( nk + (size_t)i*w, model_par( b->model_for_w2, which ), sizeof(double)*w );
    double *h[RKFD_PAR_COUNT];
    for( int k=0; k<RKFD_PAR_COUNT; k++ ) h[k] = k == which ? nk : b->h_par[k];
    if( par_upload( b, h, b->d_par, (size_t)b->par_stride ) < 0 ){ free( nk ); return -1; }
    free( b->h_par[which] ); b->h_par[which] = nk;
    b->par_gen++;
    return 0;
  }
  if( !values ) return 0;      /* no table: every key is the model's already */
  const size_t stride = rkfd_devmodel_par_stride( &b->host );
  if( (double)stride*(double)b->batch >= 2147483647.0 ){ SETERR( "rkfdBatchSetParam: the table of %d instances x %zu doubles is beyond the 2^31 doubles an instance's row offset can address", b->batch, stride ); return -1; }
  double *h[RKFD_PAR_COUNT];
  double *d = NULL;
  hipModule_t mod = NULL; hipFunction_t fn = NULL;
  int ok = 1;
  for( int k=0; k<RKFD_PAR_COUNT; k++ ) h[k] = NULL;
  for( int k=0; k<RKFD_PAR_COUNT && ok; k++ ){
    const int wk = rkfdBatchParamWidth( b, k );
    h[k] = (double *)malloc( sizeof(double)*( (size_t)b->batch*wk + 1 ) );
    if( !h[k] ){ SETERR( "rkfdBatchSetParam: out of memory" ); ok = 0; break; }
    if( k == which ) memcpy( h[k], values, sizeof(double)*(size_t)b->batch*wk );
    else for( int i=0; i<b->batch; i++ ) memcpy( h[k] + (size_t)i*wk, model_par( b->model_for_w2, k ), sizeof(double)*wk );
  }
  if( ok && hipMalloc( (void **)&d, sizeof(double)*( stride*(size_t)b->batch + 1 ) ) != hipSuccess ){
    SETERR( "rkfdBatchSetParam: cannot allocate the table on the device (%zu bytes)", sizeof(double)*stride*(size_t)b->batch ); d = NULL; ok = 0;
  }
  if( ok && par_upload( b, h, d, stride ) < 0 ) ok = 0;
  /* a batch that runs a world-specific kernel gets the one built for batches with a table */
  if( ok && b->spec_fn && spec_build( b, 1, &mod, &fn ) < 0 ) ok = 0;
  if( !ok ){
    for( int k=0; k<RKFD_PAR_COUNT; k++ ) free( h[k] );
    (void)hipFree( d );
    return -1;
  }
  for( int k=0; k<RKFD_PAR_COUNT; k++ ) b->h_par[k] = h[k];
  b->d_par = d; b->par_stride = (int)stride; b->par_gen++;
  if( fn ){ (void)hipModuleUnload( b->spec_mod ); b->spec_mod = mod; b->spec_fn = fn; b->spec_par = 1; }
  return 0;
}
extern "C" int rkfdBatchGetParam(rkfdBatch *b, int which, double *values)
{
  if( !b || !values ){ SETERR( "rkfdBatchGetParam: null argument" ); return -1; }
  const int w = rkfdBatchParamWidth( b, which );
  if( w < 0 ){ SETERR( "rkfdBatchGetParam: unknown parameter key %d (0 .. %d)", which, RKFD_PAR_COUNT-1 ); return -1; }
  if( b->d_par ) memcpy( values, b->h_par[which], sizeof(double)*(size_t)b->batch*w );
  else for( int i=0; i<b->batch; i++ ) memcpy( values + (size_t)i*w, model_par( b->model_for_w2, which ), sizeof(double)*w );
  return 0;
}
extern "C" int rkfdBatchClearParams(rkfdBatch *b)
{
  if( !b ){ SETERR( "rkfdBatchClearParams: null batch" ); return -1; }
  if( !b->d_par ) return 0;
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( par_quiesce( b ) < 0 ) return -1;
  /* (the kernel for batches without a table first: when it cannot be had, the table stays) */
  hipModule_t mod = NULL; hipFunction_t fn = NULL;
  if( b->spec_fn && spec_build( b, 0, &mod, &fn ) < 0 ) return -1;
  if( fn ){ (void)hipModuleUnload( b->spec_mod ); b->spec_mod = mod; b->spec_fn = fn; b->spec_par = 0; }
  (void)hipFree( b->d_par ); b->d_par = NULL; b->par_stride = 0; b->par_gen++;
  for( int k=0; k<RKFD_PAR_COUNT; k++ ){ free( b->h_par[k] ); b->h_par[k] = NULL; }
  return 0;
}

/* diagnostic: nsteps x rkFDUpdate with in-kernel phase stamps; out[batch][8] shader-clock cycles of
 * {kinematics, collision+penalty, sweep 2, sweep 3, MLCP, tail, unused, whole launch}.  Synchronous. */
extern "C" int rkfdBatchProfile(rkfdBatch *b, int nsteps, unsigned long long *out)
{
  if( !b || !out ){ SETERR( "rkfdBatchProfile: bad arguments" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  unsigned long long *d = NULL;
  const size_t n = sizeof(unsigned long long)*(size_t)b->batch*RKFD_NPROF;
  HIPCHK( hipMalloc( (void **)&d, n ), -1 );
  HIPCHK( hipMemset( d, 0, n ), -1 );
  b->st.prof = d;
  int r = launch( b, 0, nsteps, NULL );
  b->st.prof = NULL;
  if( r == 0 ){
    hipError_t e = hipMemcpy( out, d, n, hipMemcpyDeviceToHost );
    if( e != hipSuccess ){ SETERR( "hipMemcpy failed: %s", hipGetErrorString( e ) ); r = -1; }
  }
  (void)hipFree( d );
  return r;
}

extern "C" int rkfdBatchStatus(rkfdBatch *b, void *stream)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( join_streams( b, (hipStream_t)stream ) < 0 ) return -1;
  HIPCHK( hipStreamSynchronize( (hipStream_t)stream ), -1 );
  if( (hipStream_t)stream == b->last_stream ) b->launched = 0;
  int e = 0;
  HIPCHK( hipMemcpy( &e, b->d_err, sizeof(int), hipMemcpyDeviceToHost ), -1 );
  if( e == 1 ){
    static const char *const sname[] = { "Vert", "MLCP", "Volume" };
    SETERR( "a rigid contact occurred but no rigid solver is set up on the device for this world: plugin %s, max_rigid = %d "
            "(a batch created with max_rigid = 0 carries no rigid path; so does a plugin / world combination the device does not solve)",
            ( b->dm.solver >= 0 && b->dm.solver <= 2 ) ? sname[b->dm.solver] : "?", b->dm.maxrg );
  }
  if( e == 2 && b->dm.vol_np > 0 )
    SETERR( "contact capacity exceeded in at least one instance: more rigid pairs in volumetric contact than %d, more than %d contact-plane "
            "conditions in one pair, or more elastic contact vertices than the %d active-contact slots; what was beyond the capacity was dropped",
            b->dm.vol_np, b->dm.vol_ncp, b->dm.maxact );
  else if( e == 2 )
    SETERR( "contact capacity exceeded in at least one instance: more rigid contact vertices than max_rigid (%d), or more "
            "rigid + elastic contact vertices than the %d active-contact slots; contacts beyond the capacity were dropped", b->dm.maxrg, b->dm.maxact );
  if( e == 3 ) SETERR( "the %s plugin's QP ran out of iterations (256) or of basis history (64) in at least one instance", b->dm.vol_np > 0 ? "Volume" : "Vert" );
  if( e == 4 ) SETERR( "Volume plugin: a rigid pair the device cannot clip (a shape that is not convex, or more than 64 faces together) came into "
                       "contact in at least one instance; it was left without a contact force" );
  if( e == 5 ) SETERR( "rkfdBatchReset: at least one slot value named no row - not RKFD_RESET_KEEP, not a row of the bank (%d reserved), or "
                       "RKFD_RESET_SNAPSHOT without a snapshot; those instances were left as they were", rkfd_reset_size( b->reset ) );
  if( e != 0 ){
    /* the condition is reported once: the flag is cleared, so a later status describes what happened after this call */
    const int zero = 0;
    HIPCHK( hipMemcpy( b->d_err, &zero, sizeof(int), hipMemcpyHostToDevice ), -1 );
  }
  return e;
}

/* ---- contact statistics, snapshot / restore ---------------------------------------------------------------- */
extern "C" int rkfdBatchContactStats(rkfdBatch *b, int reset, double *mean_rigid, double *mean_elastic, long long *instance_steps)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  HIPCHK( hipDeviceSynchronize(), -1 );
  std::vector<unsigned int> h( (size_t)b->batch*4 );
  HIPCHK( hipMemcpy( h.data(), b->st.stat, sizeof(unsigned int)*h.size(), hipMemcpyDeviceToHost ), -1 );
  unsigned long long rg = 0, el = 0, n = 0;
  for( int i=0; i<b->batch; i++ ){ rg += h[4*(size_t)i]; el += h[4*(size_t)i+1]; n += h[4*(size_t)i+2]; }
  if( mean_rigid ) *mean_rigid = n ? (double)rg/(double)n : 0.0;
  if( mean_elastic ) *mean_elastic = n ? (double)el/(double)n : 0.0;
  if( instance_steps ) *instance_steps = (long long)n;
  if( reset ) HIPCHK( hipMemset( b->st.stat, 0, sizeof(unsigned int)*h.size() ), -1 );
  return 0;
}

extern "C" int rkfdBatchSnapshot(rkfdBatch *b)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  HIPCHK( hipDeviceSynchronize(), -1 );
  const size_t B = b->batch, ND = b->ndof, NL = b->nlink, NC = b->ncand;
  if( !b->has_snap ){
    int bad = 0;
    bad |= dalloc( &b->snap.dis, B*ND ); bad |= dalloc( &b->snap.vel, B*ND ); bad |= dalloc( &b->snap.acc, B*ND );
    bad |= dalloc( &b->snap.piv_type, B*NL ); bad |= dalloc( &b->snap.piv_prev, B*NL ); bad |= dalloc( &b->snap.brk, B*NL );
    bad |= dalloc( &b->snap.cv_active, B*NC ); bad |= dalloc( &b->snap.cv_type, B*NC );
    bad |= dalloc( &b->snap.cv_ref, B*NC*3 ); bad |= dalloc( &b->snap.cv_f, B*NC*3 );
    if( bad ) return -1;
    b->snap.batch = b->batch;
    b->has_snap = 1;
  }
#define SNAPCP(f, n) HIPCHK( hipMemcpy( b->snap.f, b->st.f, (n), hipMemcpyDeviceToDevice ), -1 )
  SNAPCP( dis, sizeof(double)*B*ND ); SNAPCP( vel, sizeof(double)*B*ND ); SNAPCP( acc, sizeof(double)*B*ND );
  SNAPCP( piv_type, sizeof(int)*B*NL ); SNAPCP( piv_prev, sizeof(double)*B*NL ); SNAPCP( brk, sizeof(int)*B*NL );
  SNAPCP( cv_active, sizeof(int)*B*NC ); SNAPCP( cv_type, sizeof(int)*B*NC );
  SNAPCP( cv_ref, sizeof(double)*B*NC*3 ); SNAPCP( cv_f, sizeof(double)*B*NC*3 );
#undef SNAPCP
  return 0;
}

extern "C" int rkfdBatchRestore(rkfdBatch *b, void *stream)
{
  if( !b ){ SETERR( "null batch" ); return -1; }
  if( !b->has_snap ){ SETERR( "rkfdBatchRestore: no snapshot has been taken (rkfdBatchSnapshot)" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  b->last_stream = (hipStream_t)stream; b->launched = 1;
  if( b->nsplit <= 1 ){
    hipLaunchKernelGGL( rkfd_restore_kernel, dim3( b->batch ), dim3( RKFD_WAVE ), 0, (hipStream_t)stream, b->st, b->snap, 0, b->ndof, b->nlink, b->ncand );
    HIPCHK( hipGetLastError(), -1 );
    return 0;
  }
  /* split launches: every part restores itself on its own stream, in order with its steps */
  HIPCHK( hipEventRecord( b->fork, (hipStream_t)stream ), -1 );
  for( int k=0; k<b->nsplit; k++ ){
    HIPCHK( hipStreamWaitEvent( b->sub[k], b->fork, 0 ), -1 );
    const int lo = (int)( (long long)b->batch*k/b->nsplit ), hi = (int)( (long long)b->batch*( k+1 )/b->nsplit );
    if( hi > lo ){
      hipLaunchKernelGGL( rkfd_restore_kernel, dim3( hi-lo ), dim3( RKFD_WAVE ), 0, b->sub[k], b->st, b->snap, lo, b->ndof, b->nlink, b->ncand );
      HIPCHK( hipGetLastError(), -1 );
    }
    HIPCHK( hipEventRecord( b->done[k], b->sub[k] ), -1 );
  }
  b->pending = 1;
  return 0;
}

/* ---- per-instance reset from a bank of start states ----------------------------------------------------------- */
/* the bank's object is made by the first call that needs it; it allocates nothing on the device by itself */
static int reset_object(rkfdBatch *b, const char *who)
{
  if( b->reset ) return 0;
  char err[400] = "";
  b->reset = rkfd_reset_create( b->batch, b->ndof, b->nlink, b->ncand, err, sizeof(err) );
  if( !b->reset ){ SETERR( "%s: %s", who, err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchBankSize(const rkfdBatch *b){ return b ? rkfd_reset_size( b->reset ) : -1; }
extern "C" int rkfdBatchBankReserve(rkfdBatch *b, int nslots)
{
  if( !b ){ SETERR( "rkfdBatchBankReserve: null batch" ); return -1; }
  if( nslots < 0 ){ SETERR( "rkfdBatchBankReserve: nslots must be >= 0 (got %d)", nslots ); return -1; }
  if( nslots == 0 && !b->reset ) return 0;
  HIPCHK( hipSetDevice( b->device ), -1 );
  /* a reset still queued may read the rows that go */
  if( sync_streams( b ) < 0 ) return -1;
  HIPCHK( hipDeviceSynchronize(), -1 );
  if( reset_object( b, "rkfdBatchBankReserve" ) < 0 ) return -1;
  char err[400] = "";
  if( rkfd_reset_reserve( b->reset, nslots, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchBankReserve: %s", err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchBankStore(rkfdBatch *b, int slot, int first, int count)
{
  if( !b ){ SETERR( "rkfdBatchBankStore: null batch" ); return -1; }
  if( !b->reset || rkfd_reset_size( b->reset ) == 0 ){ SETERR( "rkfdBatchBankStore: no bank has been reserved (rkfdBatchBankReserve)" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  HIPCHK( hipDeviceSynchronize(), -1 );
  char err[400] = "";
  if( rkfd_reset_store( b->reset, &b->st, slot, first, count, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchBankStore: %s", err ); return -1; }
  return 0;
}
/* slots_dev: the caller's device array, or NULL: the batch's own copy, which every part first brings over from the pinned staging
 * (as ctrl_upload does for a control schedule).  Under split launches every part resets itself on its own stream, in order with
 * its steps, as rkfdBatchRestore does. */
static int reset_launch(rkfdBatch *b, const int *slots_dev, void *stream, const char *who)
{
  char err[400] = "";
  const bool upload = slots_dev == NULL;
  if( upload ) slots_dev = rkfd_reset_dev_slots( b->reset );
  const rkfdDevState *snap = b->has_snap ? &b->snap : NULL;
  b->last_stream = (hipStream_t)stream; b->launched = 1;
  if( b->nsplit <= 1 ){
    if( ( upload && rkfd_reset_upload( b->reset, 0, b->batch, 0, stream, err, sizeof(err) ) < 0 ) ||
        rkfd_reset_launch( b->reset, &b->st, snap, slots_dev, 0, b->batch, b->d_err, stream, err, sizeof(err) ) < 0 ){ SETERR( "%s: %s", who, err ); return -1; }
    return 0;
  }
  HIPCHK( hipEventRecord( b->fork, (hipStream_t)stream ), -1 );
  for( int k=0; k<b->nsplit; k++ ){
    HIPCHK( hipStreamWaitEvent( b->sub[k], b->fork, 0 ), -1 );
    const int lo = (int)( (long long)b->batch*k/b->nsplit ), hi = (int)( (long long)b->batch*( k+1 )/b->nsplit );
    if( hi > lo && ( ( upload && rkfd_reset_upload( b->reset, lo, hi, k, b->sub[k], err, sizeof(err) ) < 0 ) ||
                     rkfd_reset_launch( b->reset, &b->st, snap, slots_dev, lo, hi, b->d_err, b->sub[k], err, sizeof(err) ) < 0 ) ){ SETERR( "%s: %s", who, err ); return -1; }
    HIPCHK( hipEventRecord( b->done[k], b->sub[k] ), -1 );
  }
  b->pending = 1;
  return 0;
}
/* the first half of rkfdBatchReset: the host array into the batch's pinned staging; nothing on the device has changed when it fails
 * (the node level stages every shard before any of them launches) */
static int reset_stage(rkfdBatch *b, const int *slots, const char *who)
{
  if( !b || !slots ){ SETERR( "%s: %s", who, !b ? "null batch" : "null slots" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( reset_object( b, who ) < 0 ) return -1;
  char err[400] = "";
  if( rkfd_reset_stage( b->reset, slots, err, sizeof(err) ) < 0 ){ SETERR( "%s: %s", who, err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchReset(rkfdBatch *b, const int *slots, void *stream)
{
  if( reset_stage( b, slots, "rkfdBatchReset" ) < 0 ) return -1;
  return reset_launch( b, NULL, stream, "rkfdBatchReset" );
}
/* the node level's route through the host (rkfdNodeBankStore): packed rows of live instances out of a batch, and into the bank of
 * another; synchronous and ordered after the batch's launches */
static int bank_rows_get(rkfdBatch *b, int first, int count, void *buf)
{
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  HIPCHK( hipDeviceSynchronize(), -1 );
  char err[400] = "";
  if( rkfd_reset_rows_get( b->reset, &b->st, first, count, buf, err, sizeof(err) ) < 0 ){ SETERR( "rkfdNodeBankStore: %s", err ); return -1; }
  return 0;
}
static int bank_rows_put(rkfdBatch *b, int slot, int count, const void *buf)
{
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( sync_streams( b ) < 0 ) return -1;
  HIPCHK( hipDeviceSynchronize(), -1 );
  char err[400] = "";
  if( rkfd_reset_rows_put( b->reset, slot, count, buf, err, sizeof(err) ) < 0 ){ SETERR( "rkfdNodeBankStore: %s", err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchResetDev(rkfdBatch *b, const int *slots_dev, void *stream)
{
  if( !b || !slots_dev ){ SETERR( "rkfdBatchResetDev: %s", !b ? "null batch" : "null slots" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( reset_object( b, "rkfdBatchResetDev" ) < 0 ) return -1;
  return reset_launch( b, slots_dev, stream, "rkfdBatchResetDev" );
}

/* ---- task-space read-out: link poses, velocities and chain COM on the device ---------------------------------- */
extern "C" int rkfdBatchLinkNum(const rkfdBatch *b){ return b ? b->nlink : -1; }
extern "C" int rkfdBatchChainNum(const rkfdBatch *b){ return b ? b->model_for_w2->nchain : -1; }
/* One launch of rkfd_links_kernel in stream order after everything the batch has launched: the internal split streams are joined
 * onto `stream` first (as rkfdBatchJoin does), no host wait.  It reads dis / vel and writes the read-out's own buffers only. */
extern "C" int rkfdBatchUpdateLinks(rkfdBatch *b, int flags, void *stream)
{
  if( !b ){ SETERR( "rkfdBatchUpdateLinks: null batch" ); return -1; }
  if( flags <= 0 || ( flags & ~( RKFD_LINKS_POSE | RKFD_LINKS_VEL | RKFD_LINKS_COM ) ) ){ SETERR( "rkfdBatchUpdateLinks: flags must be a combination of RKFD_LINKS_POSE, RKFD_LINKS_VEL and RKFD_LINKS_COM (got %d)", flags ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  char err[400] = "";
  if( !b->links ){
    b->links = rkfd_links_create( b->model_for_w2, &b->host, &b->dm, b->batch, err, sizeof(err) );
    if( !b->links ){ SETERR( "%s", err ); return -1; }
  }
  if( join_streams( b, (hipStream_t)stream ) < 0 ) return -1;
  b->last_stream = (hipStream_t)stream; b->launched = 1;
  if( rkfd_links_launch( b->links, b->st.dis, b->st.vel, flags, b->d_par ? b->h_par[RKFD_PAR_MASS] : NULL, b->d_par ? b->h_par[RKFD_PAR_COM] : NULL,
                         b->par_gen, stream, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchUpdateLinks: %s", err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchGetLinks(rkfdBatch *b, double *R, double *p, double *v, double *com, double *comvel)
{
  if( !b ){ SETERR( "rkfdBatchGetLinks: null batch" ); return -1; }
  const int have = rkfd_links_flags( b->links );
  if( !have ){ SETERR( "rkfdBatchGetLinks: no read-out has been made (rkfdBatchUpdateLinks)" ); return -1; }
  if( ( ( R || p ) && !( have & RKFD_LINKS_POSE ) ) || ( v && !( have & RKFD_LINKS_VEL ) ) || ( ( com || comvel ) && !( have & RKFD_LINKS_COM ) ) ){
    SETERR( "rkfdBatchGetLinks: the last rkfdBatchUpdateLinks (flags %d) did not compute %s", have,
            ( ( R || p ) && !( have & RKFD_LINKS_POSE ) ) ? "the poses (RKFD_LINKS_POSE)" : ( v && !( have & RKFD_LINKS_VEL ) ) ? "the velocities (RKFD_LINKS_VEL)" : "the centres of mass (RKFD_LINKS_COM)" );
    return -1;
  }
  HIPCHK( hipSetDevice( b->device ), -1 );
  char err[400] = "";
  if( rkfd_links_get( b->links, R, p, v, com, comvel, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchGetLinks: %s", err ); return -1; }
  return 0;
}
extern "C" const double *rkfdBatchDevLinkAtt(rkfdBatch *b){ return b ? rkfd_links_dev( b->links, 0 ) : NULL; }
extern "C" const double *rkfdBatchDevLinkPos(rkfdBatch *b){ return b ? rkfd_links_dev( b->links, 1 ) : NULL; }
extern "C" const double *rkfdBatchDevLinkVel(rkfdBatch *b){ return b ? rkfd_links_dev( b->links, 2 ) : NULL; }
extern "C" const double *rkfdBatchDevCom(rkfdBatch *b){ return b ? rkfd_links_dev( b->links, 3 ) : NULL; }
extern "C" const double *rkfdBatchDevComVel(rkfdBatch *b){ return b ? rkfd_links_dev( b->links, 4 ) : NULL; }

/* ---- task-space Jacobians: site and centre-of-mass Jacobians on the device ------------------------------------ */
static int jac_object(rkfdBatch *b, const char *who)
{
  if( b->jac ) return 0;
  char err[400] = "";
  b->jac = rkfd_jac_create( b->model_for_w2, b->batch, err, sizeof(err) );
  if( !b->jac ){ SETERR( "%s: %s", who, err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchSetJacobianSites(rkfdBatch *b, int nsite, const int *link, const double *point)
{
  if( !b ){ SETERR( "rkfdBatchSetJacobianSites: null batch" ); return -1; }
  char err[400] = "";
  /* (refused before anything is made or touched: the previous sites stay) */
  if( rkfd_jac_check_sites( b->nlink, nsite, link, point, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchSetJacobianSites: %s", err ); return -1; }
  if( !b->jac && nsite == 0 ) return 0;
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( jac_object( b, "rkfdBatchSetJacobianSites" ) < 0 ) return -1;
  if( rkfd_jac_set_sites( b->jac, nsite, link, point, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchSetJacobianSites: %s", err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchJacobianSiteNum(const rkfdBatch *b){ return b ? rkfd_jac_nsite( b->jac ) : -1; }
/* One launch of rkfd_jac_kernel in stream order after everything the batch has launched: the internal split streams are joined
 * onto `stream` first (as rkfdBatchJoin does), no host wait.  It reads dis and writes the Jacobians' own buffers only. */
extern "C" int rkfdBatchUpdateJacobians(rkfdBatch *b, int flags, void *stream)
{
  if( !b ){ SETERR( "rkfdBatchUpdateJacobians: null batch" ); return -1; }
  if( flags <= 0 || ( flags & ~( RKFD_JAC_SITES | RKFD_JAC_COM ) ) ){ SETERR( "rkfdBatchUpdateJacobians: flags must be a combination of RKFD_JAC_SITES and RKFD_JAC_COM (got %d)", flags ); return -1; }
  if( ( flags & RKFD_JAC_SITES ) && rkfd_jac_nsite( b->jac ) == 0 ){ SETERR( "rkfdBatchUpdateJacobians: RKFD_JAC_SITES without sites (rkfdBatchSetJacobianSites)" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  if( jac_object( b, "rkfdBatchUpdateJacobians" ) < 0 ) return -1;
  if( join_streams( b, (hipStream_t)stream ) < 0 ) return -1;
  b->last_stream = (hipStream_t)stream; b->launched = 1;
  char err[400] = "";
  if( rkfd_jac_launch( b->jac, b->st.dis, flags, b->d_par ? b->h_par[RKFD_PAR_MASS] : NULL, b->d_par ? b->h_par[RKFD_PAR_COM] : NULL,
                       b->par_gen, stream, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchUpdateJacobians: %s", err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchGetJacobians(rkfdBatch *b, double *J, double *Jcom)
{
  if( !b ){ SETERR( "rkfdBatchGetJacobians: null batch" ); return -1; }
  const int have = rkfd_jac_flags( b->jac );
  if( ( J && !( have & RKFD_JAC_SITES ) ) || ( Jcom && !( have & RKFD_JAC_COM ) ) ){
    if( !have ) SETERR( "rkfdBatchGetJacobians: no Jacobians have been computed (rkfdBatchUpdateJacobians)" );
    else SETERR( "rkfdBatchGetJacobians: the last rkfdBatchUpdateJacobians (flags %d) did not compute %s", have,
                 ( J && !( have & RKFD_JAC_SITES ) ) ? "the site Jacobians of the present sites (RKFD_JAC_SITES)" : "the centre-of-mass Jacobians (RKFD_JAC_COM)" );
    return -1;
  }
  if( !J && !Jcom ) return 0;
  HIPCHK( hipSetDevice( b->device ), -1 );
  char err[400] = "";
  if( rkfd_jac_get( b->jac, J, Jcom, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchGetJacobians: %s", err ); return -1; }
  return 0;
}
extern "C" const double *rkfdBatchDevJacobian(rkfdBatch *b){ return b ? rkfd_jac_dev( b->jac, 0 ) : NULL; }
extern "C" const double *rkfdBatchDevComJacobian(rkfdBatch *b){ return b ? rkfd_jac_dev( b->jac, 1 ) : NULL; }

/* ---- joint-space dynamics: mass matrix, bias and gravity forces on the device ---------------------------------- */
/* One launch of rkfd_dyn_kernel in stream order after everything the batch has launched: the internal split streams are joined
 * onto `stream` first (as rkfdBatchJoin does), no host wait.  It reads dis / vel and writes the dynamics' own buffers only. */
extern "C" int rkfdBatchUpdateDynamics(rkfdBatch *b, int flags, void *stream)
{
  if( !b ){ SETERR( "rkfdBatchUpdateDynamics: null batch" ); return -1; }
  if( flags <= 0 || ( flags & ~( RKFD_DYN_MASS | RKFD_DYN_BIAS | RKFD_DYN_GRAVITY | RKFD_DYN_ROTOR ) ) ){ SETERR( "rkfdBatchUpdateDynamics: flags must be a combination of RKFD_DYN_MASS, RKFD_DYN_BIAS, RKFD_DYN_GRAVITY and RKFD_DYN_ROTOR (got %d)", flags ); return -1; }
  if( ( flags & RKFD_DYN_ROTOR ) && !( flags & RKFD_DYN_MASS ) ){ SETERR( "rkfdBatchUpdateDynamics: RKFD_DYN_ROTOR without RKFD_DYN_MASS (the rotor inertia is added to the diagonal of M)" ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  char err[400] = "";
  if( !b->dyn ){
    b->dyn = rkfd_dyn_create( b->model_for_w2, b->batch, err, sizeof(err) );
    if( !b->dyn ){ SETERR( "%s", err ); return -1; }
  }
  if( join_streams( b, (hipStream_t)stream ) < 0 ) return -1;
  b->last_stream = (hipStream_t)stream; b->launched = 1;
  if( rkfd_dyn_launch( b->dyn, b->st.dis, b->st.vel, flags, b->d_par ? b->h_par[RKFD_PAR_MASS] : NULL, b->d_par ? b->h_par[RKFD_PAR_COM] : NULL,
                       b->d_par ? b->h_par[RKFD_PAR_INERTIA] : NULL, b->par_gen, stream, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchUpdateDynamics: %s", err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchGetDynamics(rkfdBatch *b, double *M, double *h, double *g)
{
  if( !b ){ SETERR( "rkfdBatchGetDynamics: null batch" ); return -1; }
  const int have = rkfd_dyn_flags( b->dyn );
  if( !have ){ SETERR( "rkfdBatchGetDynamics: no dynamics have been computed (rkfdBatchUpdateDynamics)" ); return -1; }
  if( ( M && !( have & RKFD_DYN_MASS ) ) || ( h && !( have & RKFD_DYN_BIAS ) ) || ( g && !( have & RKFD_DYN_GRAVITY ) ) ){
    SETERR( "rkfdBatchGetDynamics: the last rkfdBatchUpdateDynamics (flags %d) did not compute %s", have,
            ( M && !( have & RKFD_DYN_MASS ) ) ? "the mass matrix (RKFD_DYN_MASS)" : ( h && !( have & RKFD_DYN_BIAS ) ) ? "the bias force (RKFD_DYN_BIAS)" : "the gravity force (RKFD_DYN_GRAVITY)" );
    return -1;
  }
  if( !M && !h && !g ) return 0;
  HIPCHK( hipSetDevice( b->device ), -1 );
  char err[400] = "";
  if( rkfd_dyn_get( b->dyn, M, h, g, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchGetDynamics: %s", err ); return -1; }
  return 0;
}
extern "C" const double *rkfdBatchDevMassMatrix(rkfdBatch *b){ return b ? rkfd_dyn_dev( b->dyn, 0 ) : NULL; }
extern "C" const double *rkfdBatchDevBias(rkfdBatch *b){ return b ? rkfd_dyn_dev( b->dyn, 1 ) : NULL; }
extern "C" const double *rkfdBatchDevGravity(rkfdBatch *b){ return b ? rkfd_dyn_dev( b->dyn, 2 ) : NULL; }

/* ---- contact read-out: candidate positions, link wrenches and the generalised contact force on the device ------ */
#define CF_FLAG_NAMES "RKFD_CF_POINT, RKFD_CF_WRENCH and RKFD_CF_GENF"
/* One launch of rkfd_cf_kernel in stream order after everything the batch has launched: the internal split streams are joined onto
 * `stream` first (as rkfdBatchJoin does), no host wait.  It reads dis and the candidates' flags and forces - the batch's own or the
 * caller's - and writes the contact read-out's own buffers only. */
static int cf_launch(rkfdBatch *b, int flags, const int *active, const double *f, void *stream, const char *who)
{
  if( flags <= 0 || ( flags & ~( RKFD_CF_POINT | RKFD_CF_WRENCH | RKFD_CF_GENF ) ) ){ SETERR( "%s: flags must be a combination of " CF_FLAG_NAMES " (got %d)", who, flags ); return -1; }
  HIPCHK( hipSetDevice( b->device ), -1 );
  char err[400] = "";
  if( !b->cf ){
    b->cf = rkfd_cf_create( b->model_for_w2, b->batch, err, sizeof(err) );
    if( !b->cf ){ SETERR( "%s", err ); return -1; }
  }
  if( join_streams( b, (hipStream_t)stream ) < 0 ) return -1;
  b->last_stream = (hipStream_t)stream; b->launched = 1;
  if( rkfd_cf_launch( b->cf, b->st.dis, active, f, flags, stream, err, sizeof(err) ) < 0 ){ SETERR( "%s: %s", who, err ); return -1; }
  return 0;
}
extern "C" int rkfdBatchUpdateContactForces(rkfdBatch *b, int flags, void *stream)
{
  if( !b ){ SETERR( "rkfdBatchUpdateContactForces: null batch" ); return -1; }
  return cf_launch( b, flags, b->st.cv_active, b->st.cv_f, stream, "rkfdBatchUpdateContactForces" );
}
extern "C" int rkfdBatchUpdateContactForcesDev(rkfdBatch *b, int flags, const int *active_dev, const double *f_dev, void *stream)
{
  if( !b ){ SETERR( "rkfdBatchUpdateContactForcesDev: null batch" ); return -1; }
  if( !active_dev || !f_dev ){ SETERR( "rkfdBatchUpdateContactForcesDev: %s", !active_dev ? "null active_dev" : "null f_dev" ); return -1; }
  return cf_launch( b, flags, active_dev, f_dev, stream, "rkfdBatchUpdateContactForcesDev" );
}
extern "C" int rkfdBatchGetContactForces(rkfdBatch *b, double *point, double *wrench, int *count, double *genf)
{
  if( !b ){ SETERR( "rkfdBatchGetContactForces: null batch" ); return -1; }
  const int have = rkfd_cf_flags( b->cf );
  if( !have ){ SETERR( "rkfdBatchGetContactForces: no contact forces have been computed (rkfdBatchUpdateContactForces)" ); return -1; }
  const bool no_p = point && !( have & RKFD_CF_POINT ), no_w = ( wrench || count ) && !( have & RKFD_CF_WRENCH ), no_g = genf && !( have & RKFD_CF_GENF );
  if( no_p || no_w || no_g ){
    SETERR( "rkfdBatchGetContactForces: the last rkfdBatchUpdateContactForces (flags %d) did not compute %s", have,
            no_p ? "the candidate positions (RKFD_CF_POINT)" : no_w ? "the link wrenches and counts (RKFD_CF_WRENCH)" : "the generalised contact force (RKFD_CF_GENF)" );
    return -1;
  }
  if( !point && !wrench && !count && !genf ) return 0;
  HIPCHK( hipSetDevice( b->device ), -1 );
  char err[400] = "";
  if( rkfd_cf_get( b->cf, point, wrench, count, genf, err, sizeof(err) ) < 0 ){ SETERR( "rkfdBatchGetContactForces: %s", err ); return -1; }
  return 0;
}
extern "C" const double *rkfdBatchDevContactPoint(rkfdBatch *b){ return b ? (const double *)rkfd_cf_dev( b->cf, 0 ) : NULL; }
extern "C" const double *rkfdBatchDevContactWrench(rkfdBatch *b){ return b ? (const double *)rkfd_cf_dev( b->cf, 1 ) : NULL; }
extern "C" const int *rkfdBatchDevContactCount(rkfdBatch *b){ return b ? (const int *)rkfd_cf_dev( b->cf, 2 ) : NULL; }
extern "C" const double *rkfdBatchDevContactGenForce(rkfdBatch *b){ return b ? (const double *)rkfd_cf_dev( b->cf, 3 ) : NULL; }

#include "rkfd_capi_node.inc"      /* the node level: one host thread + stream per device, one RCCL all-gather of final states */
