/* links_driver.c - the reference-named read-out from plain C (gcc, no HIP headers): the arm falls for `steps` rkFDUpdate under
 * gravity, then rkfdChainLinkWldPos / rkfdChainLinkWldAtt of its last link and rkfdChainWldCOM are printed with the packed state
 * they belong to (tests/test_gpu_links.py puts that state into the oracle and compares).
 * build: gcc -O1 -Iinclude tests/c/links_driver.c -Lroki-fd_amd -lrkfd_amd -Wl,-rpath,$PWD/roki-fd_amd -o links_driver
 * usage: links_driver <model dir> <steps> */
#include <stdio.h>
#include <stdlib.h>
#include "roki_fd_amd.h"

static void print_vec(const char *tag, const double *x, int n)
{
  int k;
  printf( "%s", tag );
  for( k=0; k<n; k++ ) printf( " %.17g", x[k] );
  printf( "\n" );
}

int main(int argc, char *argv[])
{
  rkFD fd;
  rkFDCell *arm;
  zVec dis;
  char name[BUFSIZ];
  const char *dir = argc > 1 ? argv[1] : "models";
  const int steps = argc > 2 ? atoi( argv[2] ) : 100;
  double p[3], p2[3], R[9], com[3];
  int k, tip;

  rkFDCreate( &fd );
  snprintf( name, sizeof(name), "%s/arm_revroot.ztk", dir );
  if( !( arm = rkFDChainRegFile( &fd, name ) ) ) return 1;
  dis = zVecAlloc( rkChainJointSize( rkFDCellChain(arm) ) );
  zVecElemNC(dis,0) = 0.3; zVecElemNC(dis,1) = 0.6;
  rkFDChainSetDis( arm, dis );
  rkFDODE2Assign( &fd, Regular );
  rkFDODE2AssignRegular( &fd, RKG );
  rkFDPrpSetDT( &fd, 0.001 );
  rkFDSetSolver( &fd, MLCP );
  rkFDUpdateInit( &fd );
  if( rkFDStatus( &fd ) != 0 ) return 2;
  tip = rkChainLinkNum( rkFDCellChain(arm) ) - 1;
  /* before the first step: the frames of the initial state */
  rkfdChainLinkWldPos( rkFDCellChain(arm), tip, p );
  print_vec( "tip0", p, 3 );
  for( k=0; k<steps; k++ ){
    rkFDUpdate( &fd );
    if( rkFDStatus( &fd ) != 0 ) return 2;
  }
  rkfdChainLinkWldPos( rkFDCellChain(arm), tip, p );
  rkfdChainLinkWldAtt( rkFDCellChain(arm), tip, R );
  rkfdChainWldCOM( rkFDCellChain(arm), com );
  rkfdChainLinkWldPos( rkFDCellChain(arm), tip, p2 );      /* (the second call reuses the read-out) */
  printf( "link %d\n", tip );
  print_vec( "dis", zVecBuf(fd.dis), fd.size );
  print_vec( "vel", zVecBuf(fd.vel), fd.size );
  print_vec( "tip", p, 3 );
  print_vec( "att", R, 9 );
  print_vec( "com", com, 3 );
  printf( "%s\n", p[0] == p2[0] && p[1] == p2[1] && p[2] == p2[2] ? "reused" : "DIFFERENT" );
  rkFDUpdateDestroy( &fd );
  zVecFree( dis );
  rkFDDestroy( &fd );
  return 0;
}
