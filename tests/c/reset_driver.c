/* reset_driver.c - the per-instance reset from plain C (gcc, no HIP headers): the batch calls are those of rkfd_hip.h alone (the world
 * comes from the builder of roki_fd_amd.h, as in node_driver.c).  Config 4's world, `batch` instances that drop from their own
 * heights: steps, rkfdBatchBankStore of instance 1, rkfdBatchReset of instance 0 from that row while the others run on, steps -
 * instance 0 must then equal instance 1 bit for bit, the others must equal a second batch that was never reset; a slot value that
 * names no row is reported once as status 5.
 * build: gcc -O1 -Iinclude tests/c/reset_driver.c -Lroki-fd_amd -lrkfd_amd -Wl,-rpath,$PWD/roki-fd_amd -o reset_driver
 * usage: reset_driver <model dir> <batch >= 3> <steps> */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "roki_fd_amd.h"
#include "rkfd_hip.h"

#define CHK(call) do{ if( (call) < 0 ){ fprintf( stderr, "%s: %s\n", #call, rkfdHipLastError() ); return 2; } }while(0)

int main(int argc, char *argv[])
{
  const char *dir = argc > 1 ? argv[1] : "models";
  const int B = argc > 2 ? atoi( argv[2] ) : 6, steps = argc > 3 ? atoi( argv[3] ) : 10;
  char name[1024];
  rkfdWorldHandle *w = rkfdWorldCreate();
  const rkfdModel *m;
  rkfdBatch *b[2];
  double *dis, *vel, *init, *x[2][3];
  int *slots;
  int h, i, k, q, nd, st, same;

  if( B < 3 ) return 1;
  snprintf( name, sizeof(name), "%s/contact_rigid.ztk", dir );
  if( rkfdWorldSetContactInfo( w, name ) != 0 ) return 1;
  snprintf( name, sizeof(name), "%s/humanoid30.ztk", dir );
  if( ( h = rkfdWorldRegFile( w, name ) ) < 0 ) return 1;
  snprintf( name, sizeof(name), "%s/floor.ztk", dir );
  if( rkfdWorldRegFile( w, name ) < 0 ) return 1;
  rkfdWorldPairChainUnreg( w, h );
  rkfdWorldSetPrp( w, 0.001, 100.0, 10, RKFD_SOLVER_MLCP );
  if( !( m = rkfdWorldModel( w ) ) ) return 1;
  nd = m->ndof;

  dis = (double *)calloc( (size_t)B*nd, sizeof(double) ); vel = (double *)calloc( (size_t)B*nd, sizeof(double) );
  init = (double *)calloc( (size_t)nd, sizeof(double) );
  slots = (int *)calloc( (size_t)B, sizeof(int) );
  for( q=0; q<2; q++ ) for( k=0; k<3; k++ ) x[q][k] = (double *)calloc( (size_t)B*nd, sizeof(double) );
  rkfdWorldChainInitDis( w, h, init );
  for( i=0; i<B; i++ ){
    memcpy( dis + (size_t)i*nd, init, sizeof(double)*nd );
    dis[(size_t)i*nd+2] += 0.002*( i % 7 );          /* every instance drops from its own height */
    dis[(size_t)i*nd+8] += 0.01*( i % 5 );
  }
  printf( "bank of a null batch %d\n", rkfdBatchBankSize( NULL ) );
  for( q=0; q<2; q++ ){
    if( !( b[q] = rkfdBatchCreate( m, B, 0, 8 ) ) ){ fprintf( stderr, "rkfdBatchCreate: %s\n", rkfdHipLastError() ); return 2; }
    CHK( rkfdBatchSetState( b[q], dis, vel ) );
    CHK( rkfdBatchUpdateInit( b[q], NULL ) );
    CHK( rkfdBatchUpdate( b[q], steps, NULL ) );
  }
  printf( "bank before %d\n", rkfdBatchBankSize( b[0] ) );
  CHK( rkfdBatchBankReserve( b[0], 2 ) );
  CHK( rkfdBatchBankStore( b[0], 1, 1, 1 ) );
  printf( "bank %d\n", rkfdBatchBankSize( b[0] ) );
  for( i=0; i<B; i++ ) slots[i] = RKFD_RESET_KEEP;
  slots[0] = 1;
  CHK( rkfdBatchReset( b[0], slots, NULL ) );
  slots[0] = 77;                                      /* (the staging was taken before the call returned) */
  for( q=0; q<2; q++ ) CHK( rkfdBatchUpdate( b[q], steps, NULL ) );
  for( q=0; q<2; q++ ){
    if( ( st = rkfdBatchStatus( b[q], NULL ) ) != 0 ){ fprintf( stderr, "status %d: %s\n", st, rkfdHipLastError() ); return 2; }
    CHK( rkfdBatchGetState( b[q], x[q][0], x[q][1], x[q][2] ) );
  }
  same = 1;
  for( k=0; k<3; k++ ) same = same && memcmp( x[0][k], x[0][k] + nd, sizeof(double)*nd ) == 0;
  printf( "twin %s\n", same ? "identical" : "DIFFERENT" );
  same = 1;
  for( k=0; k<3; k++ ) same = same && memcmp( x[0][k] + nd, x[1][k] + nd, sizeof(double)*nd*( B-1 ) ) == 0;
  printf( "others %s\n", same ? "identical" : "DIFFERENT" );
  printf( "reset instance %s\n", memcmp( x[0][0], x[1][0], sizeof(double)*nd ) != 0 ? "moved" : "UNMOVED" );
  /* a value that names no row: 2 is beyond the bank; SNAPSHOT without a snapshot */
  slots[0] = RKFD_RESET_KEEP; slots[2] = 2;
  CHK( rkfdBatchReset( b[0], slots, NULL ) );
  printf( "status %d", rkfdBatchStatus( b[0], NULL ) );
  printf( " then %d\n", rkfdBatchStatus( b[0], NULL ) );
  slots[2] = RKFD_RESET_SNAPSHOT;
  CHK( rkfdBatchReset( b[0], slots, NULL ) );
  printf( "status %d\n", rkfdBatchStatus( b[0], NULL ) );
  CHK( rkfdBatchGetState( b[0], x[1][0], x[1][1], x[1][2] ) );
  same = 1;
  for( k=0; k<3; k++ ) same = same && memcmp( x[0][k], x[1][k], sizeof(double)*nd*B ) == 0;
  printf( "after bad values %s\n", same ? "untouched" : "CHANGED" );
  CHK( rkfdBatchBankReserve( b[0], 0 ) );
  printf( "bank freed %d\n", rkfdBatchBankSize( b[0] ) );
  for( q=0; q<2; q++ ) rkfdBatchDestroy( b[q] );
  rkfdWorldFree( w );
  free( dis ); free( vel ); free( init ); free( slots );
  for( q=0; q<2; q++ ) for( k=0; k<3; k++ ) free( x[q][k] );
  return 0;
}
