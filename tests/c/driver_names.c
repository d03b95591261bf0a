/* driver_names.c - a driver in the shape of the reference's example drivers, through <roki_fd/roki_fd.h>: the names those
 * drivers use that the programs under examples/ do not (rkChainLinkNum, rkFDDT, zRandInit, zVecFPrint, zVecFreeAtOnce).
 * tests/test_loader.py compiles it with -Werror=implicit-function-declaration and links it against librkfd_amd.so.
 * usage: ./driver_names <model dir> [steps]
 */
#include <stdio.h>
#include <roki_fd/roki_fd.h>

int main(int argc, char *argv[])
{
  rkFD fd;
  rkFDCell *lc;
  zVec dis, vel;
  int i, steps;
  char name[BUFSIZ];

  if( argc < 2 ) return 1;
  steps = argc > 2 ? atoi( argv[2] ) : 10;
  zRandInit();
  rkFDCreate( &fd );
  snprintf( name, sizeof(name), "%s/box.ztk", argv[1] );
  if( !( lc = rkFDChainRegFile( &fd, name ) ) ) return 1;
  snprintf( name, sizeof(name), "%s/floor.ztk", argv[1] );
  if( !rkFDChainRegFile( &fd, name ) ) return 1;
  dis = zVecAlloc( rkChainJointSize( rkFDCellChain(lc) ) );
  vel = zVecAlloc( rkChainJointSize( rkFDCellChain(lc) ) );
  rkFDODE2Assign( &fd, Regular );
  rkFDODE2AssignRegular( &fd, RKG );
  rkFDPrpSetDT( &fd, 0.001 );
  rkFDSetSolver( &fd, Volume );
  rkFDUpdateInit( &fd );
  for( i=0; i<steps && rkFDTime(&fd) < steps*rkFDDT(&fd); i++ )
    rkFDUpdate( &fd );
  rkFDUpdateDestroy( &fd );
  printf( "links %d\n", rkChainLinkNum( rkFDCellChain(lc) ) );
  rkChainGetJointDisAll( rkFDCellChain(lc), dis );
  zVecFPrint( stdout, dis );
  zVecFreeAtOnce( 2, dis, vel );
  rkFDDestroy( &fd );
  return 0;
}
