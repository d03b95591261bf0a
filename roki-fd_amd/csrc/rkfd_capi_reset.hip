/* rkfd_capi_reset.hip - the per-instance reset behind rkfdBatchBankReserve / BankStore / Reset / ResetDev (include/rkfd_hip.h): a
 * bank of start states on the batch's device, laid out as an rkfdDevState of nslots instances, and one kernel that gives every
 * instance what its slot value says (reset/rkfd_reset.h): a row of the bank, its own row of the whole-batch snapshot, or nothing.
 * A translation unit of its own, as rkfd_capi_links.hip is: the step kernels of rkfd_capi.hip stay what they are to the
 * instruction; this kernel's resource report goes to kernel_resources_reset.txt. */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "reset/rkfd_reset.h"
#include "reset/rkfd_reset_host.h"

/* one instance per wavefront, RKFD_RESET_WAVES of them per workgroup, over the instances [first, end); a wavefront beyond `end`
 * (the last, partial workgroup) returns on its own, as does one whose instance keeps its state: there is no workgroup barrier.
 * The common call of an RL loop resets a percent of the batch, so nearly every wavefront is one load and one scalar branch. */
extern "C" __global__ void __launch_bounds__(RKFD_WAVE*RKFD_RESET_WAVES)
rkfd_reset_kernel(rkfdDevState st, rkfdDevState bank, rkfdDevState snap, const int *slots, int first, int end, int nslots, int has_snap,
                  int ND, int NL, int NC, int *errflag)
{
  const int tid = (int)threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane( tid >> 6 ), lane = tid & ( RKFD_WAVE-1 );
  rkfd_reset_wavefront( st, bank, nslots, snap, has_snap, slots, first, end, blockIdx.x, wave, lane, ND, NL, NC, errflag );
}

#define RFAIL(...) do{ if( err ) snprintf( err, errlen, __VA_ARGS__ ); return -1; }while(0)
#define RHIP(call) do{ hipError_t e_ = (call); if( e_ != hipSuccess ) RFAIL( "%s failed: %s", #call, hipGetErrorString( e_ ) ); }while(0)

struct rkfdReset {
  int batch, ND, NL, NC;
  int nslots;
  rkfdDevState bank;      /* nslots rows on the device (the pointers a row has; the others stay NULL) */
  /* rkfdBatchReset's host array: pinned staging and its device copy (made by the first call), and per part the event that marks
   * the end of the launch that read its block: the next call waits for them before it overwrites the staging and the copy */
  int *h_slots, *d_slots;
  hipEvent_t up_ev[RKFD_RESET_MAX_PARTS];
  int up_rec[RKFD_RESET_MAX_PARTS];
  int up_part;            /* the part whose upload is queued and whose launch comes next (-1: none) */
};

extern "C" rkfdReset *rkfd_reset_create(int batch, int ND, int NL, int NC, char *err, int errlen)
{
  rkfdReset *r = (rkfdReset *)calloc( 1, sizeof(rkfdReset) );
  if( !r ){ if( err ) snprintf( err, errlen, "out of memory" ); return NULL; }
  r->batch = batch; r->ND = ND; r->NL = NL; r->NC = NC; r->up_part = -1;
  return r;
}

static void bank_free(rkfdReset *r)
{
  rkfdDevState &k = r->bank;
  (void)hipFree( k.dis ); (void)hipFree( k.vel ); (void)hipFree( k.acc );
  (void)hipFree( k.piv_type ); (void)hipFree( k.piv_prev ); (void)hipFree( k.brk );
  (void)hipFree( k.cv_active ); (void)hipFree( k.cv_type ); (void)hipFree( k.cv_ref ); (void)hipFree( k.cv_f );
  memset( &k, 0, sizeof(k) );
  r->nslots = 0;
}

extern "C" void rkfd_reset_destroy(rkfdReset *r)
{
  if( !r ) return;
  for( int k=0; k<RKFD_RESET_MAX_PARTS; k++ )
    if( r->up_ev[k] ){ if( r->up_rec[k] ) (void)hipEventSynchronize( r->up_ev[k] ); (void)hipEventDestroy( r->up_ev[k] ); }
  bank_free( r );
  (void)hipFree( r->d_slots );
  if( r->h_slots ) (void)hipHostFree( r->h_slots );
  free( r );
}

extern "C" int rkfd_reset_size(const rkfdReset *r){ return r ? r->nslots : 0; }

template<class T> static int bank_alloc(T **p, size_t n){ return hipMalloc( (void **)p, sizeof(T)*( n ? n : 1 ) ) == hipSuccess ? 0 : -1; }

extern "C" int rkfd_reset_reserve(rkfdReset *r, int nslots, char *err, int errlen)
{
  bank_free( r );
  if( nslots == 0 ) return 0;
  const size_t S = (size_t)nslots, ND = r->ND, NL = r->NL, NC = r->NC;
  rkfdDevState &k = r->bank;
  int bad = 0;
  bad |= bank_alloc( &k.dis, S*ND ); bad |= bank_alloc( &k.vel, S*ND ); bad |= bank_alloc( &k.acc, S*ND );
  bad |= bank_alloc( &k.piv_type, S*NL ); bad |= bank_alloc( &k.piv_prev, S*NL ); bad |= bank_alloc( &k.brk, S*NL );
  bad |= bank_alloc( &k.cv_active, S*NC ); bad |= bank_alloc( &k.cv_type, S*NC );
  bad |= bank_alloc( &k.cv_ref, S*NC*3 ); bad |= bank_alloc( &k.cv_f, S*NC*3 );
  if( bad ){
    (void)hipGetLastError();
    bank_free( r );
    RFAIL( "cannot allocate a bank of %d start states on the device", nslots );
  }
  k.batch = nslots;
  r->nslots = nslots;
  return 0;
}

/* `count` rows from row `srow` of src to row `drow` of dst, array by array */
static int rows_copy(const rkfdReset *r, const rkfdDevState &dst, size_t drow, const rkfdDevState &src, size_t srow, size_t count,
                     hipMemcpyKind kind, char *err, int errlen)
{
  const size_t ND = r->ND, NL = r->NL, NC = r->NC;
#define ROWCP(f, w) do{ if( (w)*count ) RHIP( hipMemcpy( dst.f + drow*(w), src.f + srow*(w), sizeof(*dst.f)*(w)*count, kind ) ); }while(0)
  ROWCP( dis, ND ); ROWCP( vel, ND ); ROWCP( acc, ND );
  ROWCP( piv_type, NL ); ROWCP( piv_prev, NL ); ROWCP( brk, NL );
  ROWCP( cv_active, NC ); ROWCP( cv_type, NC ); ROWCP( cv_ref, 3*NC ); ROWCP( cv_f, 3*NC );
#undef ROWCP
  return 0;
}

static int range_check(const rkfdReset *r, int slot, int first, int count, char *err, int errlen)
{
  if( count < 1 ) RFAIL( "count must be >= 1 (got %d)", count );
  if( slot < 0 || (long long)slot + count > r->nslots ) RFAIL( "rows %d .. %d are not within the bank of %d (rkfdBatchBankReserve)", slot, slot+count-1, r->nslots );
  if( first < 0 || (long long)first + count > r->batch ) RFAIL( "instances %d .. %d are not within the batch of %d", first, first+count-1, r->batch );
  return 0;
}

extern "C" int rkfd_reset_store(rkfdReset *r, const rkfdDevState *st, int slot, int first, int count, char *err, int errlen)
{
  if( range_check( r, slot, first, count, err, errlen ) < 0 ) return -1;
  if( rows_copy( r, r->bank, (size_t)slot, *st, (size_t)first, (size_t)count, hipMemcpyDeviceToDevice, err, errlen ) < 0 ) return -1;
  /* (a copy within the device may return before it is done, and a stream made with hipStreamNonBlocking is not ordered after it) */
  RHIP( hipDeviceSynchronize() );
  return 0;
}

/* `count` packed rows in a host buffer, seen as an rkfdDevState: the arrays of doubles first */
static rkfdDevState host_rows(const rkfdReset *r, void *buf, size_t count)
{
  const size_t ND = r->ND, NL = r->NL, NC = r->NC;
  rkfdDevState h;
  memset( &h, 0, sizeof(h) );
  double *d = (double *)buf;
  h.dis = d; d += count*ND; h.vel = d; d += count*ND; h.acc = d; d += count*ND;
  h.piv_prev = d; d += count*NL; h.cv_ref = d; d += count*3*NC; h.cv_f = d; d += count*3*NC;
  int *i = (int *)d;
  h.piv_type = i; i += count*NL; h.brk = i; i += count*NL; h.cv_active = i; i += count*NC; h.cv_type = i;
  h.batch = (int)count;
  return h;
}
extern "C" size_t rkfd_reset_row_bytes(const rkfdReset *r, int count)
{
  const size_t ND = r->ND, NL = r->NL, NC = r->NC;
  return (size_t)( count > 0 ? count : 0 )*( sizeof(double)*( 3*ND + NL + 6*NC ) + sizeof(int)*( 2*NL + 2*NC ) );
}
extern "C" int rkfd_reset_rows_get(rkfdReset *r, const rkfdDevState *st, int first, int count, void *buf, char *err, int errlen)
{
  if( count < 1 || first < 0 || (long long)first + count > r->batch ) RFAIL( "instances %d .. %d are not within the batch of %d", first, first+count-1, r->batch );
  return rows_copy( r, host_rows( r, buf, (size_t)count ), 0, *st, (size_t)first, (size_t)count, hipMemcpyDeviceToHost, err, errlen );
}
extern "C" int rkfd_reset_rows_put(rkfdReset *r, int slot, int count, const void *buf, char *err, int errlen)
{
  if( count < 1 || slot < 0 || (long long)slot + count > r->nslots ) RFAIL( "rows %d .. %d are not within the bank of %d (rkfdBatchBankReserve)", slot, slot+count-1, r->nslots );
  if( rows_copy( r, r->bank, (size_t)slot, host_rows( r, (void *)buf, (size_t)count ), 0, (size_t)count, hipMemcpyHostToDevice, err, errlen ) < 0 ) return -1;
  RHIP( hipDeviceSynchronize() );
  return 0;
}

extern "C" int rkfd_reset_stage(rkfdReset *r, const int *slots, char *err, int errlen)
{
  const size_t n = (size_t)r->batch;
  if( !r->h_slots ){
    int *h = NULL, *d = NULL;
    if( hipHostMalloc( (void **)&h, sizeof(int)*n, hipHostMallocDefault ) != hipSuccess || hipMalloc( (void **)&d, sizeof(int)*n ) != hipSuccess ){
      (void)hipGetLastError();
      if( h ) (void)hipHostFree( h );
      RFAIL( "cannot allocate the staging of %zu slot values", n );
    }
    for( int k=0; k<RKFD_RESET_MAX_PARTS; k++ )
      if( !r->up_ev[k] && hipEventCreateWithFlags( &r->up_ev[k], hipEventDisableTiming ) != hipSuccess ){
        (void)hipHostFree( h ); (void)hipFree( d );
        RFAIL( "hipEventCreate failed" );
      }
    r->h_slots = h; r->d_slots = d;
  }
  /* the staging may still feed the uploads of the previous call, and its launches may still read the device copy */
  for( int k=0; k<RKFD_RESET_MAX_PARTS; k++ )
    if( r->up_rec[k] ){ RHIP( hipEventSynchronize( r->up_ev[k] ) ); r->up_rec[k] = 0; }
  memcpy( r->h_slots, slots, sizeof(int)*n );
  return 0;
}

extern "C" int rkfd_reset_upload(rkfdReset *r, int lo, int hi, int part, void *stream, char *err, int errlen)
{
  if( !r->h_slots || part < 0 || part >= RKFD_RESET_MAX_PARTS || lo < 0 || hi > r->batch || hi <= lo ) RFAIL( "rkfd_reset_upload: bad arguments" );
  RHIP( hipMemcpyAsync( r->d_slots + lo, r->h_slots + lo, sizeof(int)*(size_t)( hi-lo ), hipMemcpyHostToDevice, (hipStream_t)stream ) );
  r->up_part = part;
  return 0;
}

extern "C" const int *rkfd_reset_dev_slots(const rkfdReset *r){ return r ? r->d_slots : NULL; }

extern "C" int rkfd_reset_launch(rkfdReset *r, const rkfdDevState *st, const rkfdDevState *snap, const int *slots_dev, int lo, int hi,
                                 int *errflag, void *stream, char *err, int errlen)
{
  if( lo < 0 || hi > r->batch || hi <= lo || !slots_dev ) RFAIL( "rkfd_reset_launch: bad arguments" );
  rkfdDevState none;
  memset( &none, 0, sizeof(none) );
  const unsigned blocks = (unsigned)( ( (size_t)( hi-lo ) + RKFD_RESET_WAVES - 1 )/RKFD_RESET_WAVES );
  hipLaunchKernelGGL( rkfd_reset_kernel, dim3( blocks ), dim3( RKFD_WAVE*RKFD_RESET_WAVES ), 0, (hipStream_t)stream,
                      *st, r->bank, snap ? *snap : none, slots_dev, lo, hi, r->nslots, snap ? 1 : 0, r->ND, r->NL, r->NC, errflag );
  RHIP( hipGetLastError() );
  if( slots_dev == r->d_slots && r->up_part >= 0 ){
    /* the launch read the batch's own copy: the next host array waits for it before it takes the staging and the copy */
    RHIP( hipEventRecord( r->up_ev[r->up_part], (hipStream_t)stream ) );
    r->up_rec[r->up_part] = 1; r->up_part = -1;
  }
  return 0;
}
