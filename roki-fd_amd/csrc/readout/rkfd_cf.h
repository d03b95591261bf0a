/* rkfd_cf.h - contact read-out (rkfdBatchUpdateContactForces): the contact term J_c' f of the equation of motion of one instance,
 * from its live dis and the force of every candidate contact vertex - the world position of every candidate vertex, the net contact
 * wrench and the number of active candidates of every model link, and the generalised contact force on the packed joint rates.  One
 * instance per 64-lane wavefront; compiles for gfx950 (rkfd_capi_cf.hip) and under the lane emulator (tests/emu/rkfd_emu_cf.cpp).
 * Like the read-out, the Jacobians and the dynamics it is no part of the step kernels: it reads dis, the flags and forces of the
 * candidates and the model's tables, writes its own buffers, and lives outside csrc/device/.
 *
 * It works in MODEL space with the adjacent maps ( E, B ) and the unit twists of rkfd_jac.h, and walks the tree with rkfd_jac_walk:
 * genf is by construction sum_l J_l' ( F_l, N_l ) with J_l the site Jacobian of ( link l, its origin ) as rkfdBatchUpdateJacobians
 * gives it.
 *   1. lane = model link, 64 at a time: ( E_i, B_i ) and the unit twists S_c into LDS (phase 1 of rkfd_jac_instance restated, as
 *      rkfd_dyn.h restates it: it is no function of its own there, and that kernel's source stays untouched), and the
 *      parent-frame position pa_i of the link origin; then every lane composes its link's world pose R_i, p_i on its own way up to the
 *      root, R <- Ra_a R, p <- Ra_a p + pa_a, into LDS.
 *   2. lane = candidate, 64 at a time: x_j = p_own + R_own v_j, active or not, stored as `point`.
 *   3. one scalar per lane over ( link, component ), strided: the lane scans the link's list of ( candidate, sign ) IN CANDIDATE INDEX
 *      ORDER (host-built, CSR), recomputes x_j from the owner's pose, reads the flag and f_j from global memory and sums its own
 *      component of ( +-f_j, ( x_j - p_link ) x +-f_j ) in its own register.  A candidate whose flag is 0 is SKIPPED (never multiplied
 *      by the flag: the step kernel leaves stale values there, a caller may leave NaN).  wrench and count go to LDS and to global memory.
 *   4. lane = coordinate c: over the links in index order, skipping a link no active candidate touches (the same for all lanes), the
 *      walk from the link to its root; genf[c] += J_l[0:3, c] . F_l + J_l[3:6, c] . N_l where the walk passed the owner of c.  Lanes
 *      whose owner is never passed keep an exact 0.0.
 * No atomics, no cross-lane reduction: the same bits every launch.  No mass and no other per-instance parameter enters.
 *
 * Conventions of the results: point [ncand][3] world; wrench [nlink][6] world axes, rows 0-2 the force, rows 3-5 the moment about the
 * link's own origin; an active candidate j gives +f_j at x_j to the link that owns the vertex and -f_j at x_j to the other link of
 * its pair; count [nlink] active candidates that touch the link on either side; genf [ndof] on the coordinates of the columns of J. */
#ifndef RKFD_CF_H
#define RKFD_CF_H

#include "readout/rkfd_jac.h"

#define RKFD_CF_F_POINT  1
#define RKFD_CF_F_WRENCH 2
#define RKFD_CF_F_GENF   4
#define RKFD_CF_MAX_WAVES 4      /* instances (wavefronts) of one workgroup, at most: 4, 2 or 1 by the LDS one instance needs */

/* every pointer a device pointer (host under the emulator); all tables in MODEL space */
typedef struct {
  rkfdJacTab j;                           /* nlink, ndof, parent, jtype, dofoff, org, cown: what phase 1 and rkfd_jac_walk read */
  int ncand;
  const int *c_own, *c_oth;               /* [ncand] the link that owns the vertex, the other link of the pair */
  const double *c_vert;                   /* [ncand*3] the vertex in the owner's frame */
  const int *l_off, *l_ent;               /* [nlink+1], [2 ncand]: the candidates of a link in index order, 2 x candidate + ( 1: the link is the other side ) */
} rkfdCfTab;

/* doubles of LDS one instance takes: ( E, B ) of every model link (18), the unit twists of the coordinates (6 each), per link pa (3),
 * the world pose (12), the wrench (6) and the count (an int in a slot of its own) */
#define RKFD_CF_LDS_DOUBLES(NLM, ND) ( 40*(NLM) + 6*(ND) )

RKFD_DEV void rkfd_cf_instance(const rkfdCfTab &t, const double *dis, const int *active, const double *f, size_t b, int lane, double *lds, int flags,
                               double *opoint, double *owrench, int *ocount, double *ogenf)
{
  const rkfdJacTab &tj = t.j;
  const int NLM = tj.nlink, ND = tj.ndof, NC = t.ncand;
  double *AE = lds, *AB = AE + 9*NLM, *SC = AB + 9*NLM, *PA = SC + 6*ND, *WR = PA + 3*NLM, *WP = WR + 9*NLM, *WF = WP + 3*NLM;
  int *CNT = (int *)( WF + 6*NLM );
  const double *q = dis + b*ND;
  const int *act = active + b*(size_t)NC;
  const double *fc = f + b*(size_t)NC*3;

  /* 1. lane = model link: the adjacent map ( E, B ) = ( Ra', Ra' C(pa) ), Ra = org frame x joint transform, the unit twists and pa */
  for( int j0=0; j0<NLM; j0+=RKFD_WAVE ){
    const int j = j0 + lane;
    const bool on = j < NLM;
    const int jj = on ? j : 0;
    const int jt = on ? tj.jtype[jj] : RKFD_JOINT_FIXED;
    const int off = tj.dofoff[jj];
    double o[12], Ra[9], pa[3], Rj[9] = { 1,0,0, 0,1,0, 0,0,1 };
#pragma unroll
    for( int k=0; k<12; k++ ) o[k] = tj.org[12*jj+k];
#pragma unroll
    for( int k=0; k<9; k++ ) Ra[k] = o[k];
    pa[0] = o[9]; pa[1] = o[10]; pa[2] = o[11];
    if( jt == RKFD_JOINT_REVOL ){
      double s, c;
      d_sincos( q[off], &s, &c );
      const double Rz[9] = { c,-s,0, s,c,0, 0,0,1 };
      d_mul33( o, Rz, Ra );
    } else if( jt == RKFD_JOINT_PRISM ){
      const double q1 = q[off];
      pa[0] += q1*o[2]; pa[1] += q1*o[5]; pa[2] += q1*o[8];
    } else if( jt == RKFD_JOINT_FLOAT || jt == RKFD_JOINT_BRFLOAT ){
      double qq[6], tt[3];
#pragma unroll
      for( int k=0; k<6; k++ ) qq[k] = q[off+k];
      d_from_aa( qq+3, Rj );
      d_mul33( o, Rj, Ra );
      d_mulv( o, qq, tt );
      pa[0] += tt[0]; pa[1] += tt[1]; pa[2] += tt[2];
    } else if( jt == RKFD_JOINT_SPHER ){
      const double aa[3] = { q[off], q[off+1], q[off+2] };
      d_from_aa( aa, Rj );
      d_mul33( o, Rj, Ra );
    }
    if( on ){
      const double Cx[9] = { 0, pa[2], -pa[1], -pa[2], 0, pa[0], pa[1], -pa[0], 0 };
      const double Rat[9] = { Ra[0],Ra[3],Ra[6], Ra[1],Ra[4],Ra[7], Ra[2],Ra[5],Ra[8] };
      double Bv[9];
      d_mul33( Rat, Cx, Bv );
#pragma unroll
      for( int k=0; k<9; k++ ){ AE[9*j+k] = Rat[k]; AB[9*j+k] = Bv[k]; }
      PA[3*j] = pa[0]; PA[3*j+1] = pa[1]; PA[3*j+2] = pa[2];
      /* S of the link's coordinates, (linear, angular) in the link's frame: Rj' e_k is row k of Rj */
      if( jt == RKFD_JOINT_REVOL || jt == RKFD_JOINT_PRISM ){
#pragma unroll
        for( int k=0; k<6; k++ ) SC[6*off+k] = 0;
        SC[6*off + ( jt == RKFD_JOINT_REVOL ? 5 : 2 )] = 1.0;
      } else if( jt == RKFD_JOINT_FLOAT || jt == RKFD_JOINT_BRFLOAT ){
#pragma unroll
        for( int k=0; k<3; k++ )
#pragma unroll
          for( int x=0; x<3; x++ ){
            SC[6*(off+k)+x] = Rj[3*k+x]; SC[6*(off+k)+3+x] = 0;
            SC[6*(off+3+k)+x] = 0; SC[6*(off+3+k)+3+x] = Rj[3*k+x];
          }
      } else if( jt == RKFD_JOINT_SPHER ){
#pragma unroll
        for( int k=0; k<3; k++ )
#pragma unroll
          for( int x=0; x<3; x++ ){ SC[6*(off+k)+x] = 0; SC[6*(off+k)+3+x] = Rj[3*k+x]; }
      }
    }
  }
  SYNC();

  /* the world pose of every link: the lane composes its own link's on the way up, Ra_a = E_a' */
  for( int j=lane; j<NLM; j+=RKFD_WAVE ){
    double R[9], p[3] = { PA[3*j], PA[3*j+1], PA[3*j+2] };
#pragma unroll
    for( int r=0; r<3; r++ )
#pragma unroll
      for( int c=0; c<3; c++ ) R[3*r+c] = AE[9*j+3*c+r];
    for( int a=tj.parent[j]; a>=0; a=tj.parent[a] ){
      double Ea[9], T[9];
#pragma unroll
      for( int k=0; k<9; k++ ) Ea[k] = AE[9*a+k];
      d_tmulv( Ea, p, p );
      p[0] += PA[3*a]; p[1] += PA[3*a+1]; p[2] += PA[3*a+2];
#pragma unroll
      for( int r=0; r<3; r++ )
#pragma unroll
        for( int c=0; c<3; c++ ) T[3*r+c] = Ea[r]*R[c] + Ea[3+r]*R[3+c] + Ea[6+r]*R[6+c];
#pragma unroll
      for( int k=0; k<9; k++ ) R[k] = T[k];
    }
#pragma unroll
    for( int k=0; k<9; k++ ) WR[9*j+k] = R[k];
    WP[3*j] = p[0]; WP[3*j+1] = p[1]; WP[3*j+2] = p[2];
  }
  SYNC();

  /* 2. lane = candidate: the world position of its vertex */
  if( flags & RKFD_CF_F_POINT ){
    for( int j=lane; j<NC; j+=RKFD_WAVE ){
      const int own = t.c_own[j];
      const double v[3] = { t.c_vert[3*j], t.c_vert[3*j+1], t.c_vert[3*j+2] };
      double x[3];
      d_mulv( WR + 9*own, v, x );
      double *dst = opoint + ( b*(size_t)NC + j )*3;
      dst[0] = WP[3*own] + x[0]; dst[1] = WP[3*own+1] + x[1]; dst[2] = WP[3*own+2] + x[2];
    }
  }
  if( !( flags & ( RKFD_CF_F_WRENCH | RKFD_CF_F_GENF ) ) ) return;

  /* 3. one component of one link's wrench per lane, the link's candidates in index order */
  for( int s=lane; s<6*NLM; s+=RKFD_WAVE ){
    const int l = s/6, k = s - 6*l;
    const double pl[3] = { WP[3*l], WP[3*l+1], WP[3*l+2] };
    double acc = 0;
    int cnt = 0;
    for( int e=t.l_off[l]; e<t.l_off[l+1]; e++ ){
      const int ent = t.l_ent[e], j = ent >> 1;
      if( act[j] == 0 ) continue;
      const int own = t.c_own[j];
      const double v[3] = { t.c_vert[3*j], t.c_vert[3*j+1], t.c_vert[3*j+2] };
      const double fj[3] = { fc[3*j], fc[3*j+1], fc[3*j+2] };
      double x[3], n[3];
      d_mulv( WR + 9*own, v, x );
      x[0] += WP[3*own] - pl[0]; x[1] += WP[3*own+1] - pl[1]; x[2] += WP[3*own+2] - pl[2];
      d_cross( x, fj, n );
      const double val = k == 0 ? fj[0] : k == 1 ? fj[1] : k == 2 ? fj[2] : k == 3 ? n[0] : k == 4 ? n[1] : n[2];
      acc += ( ent & 1 ) ? -val : val;
      cnt++;
    }
    WF[s] = acc;
    if( k == 0 ) CNT[l] = cnt;
    if( flags & RKFD_CF_F_WRENCH ){
      owrench[b*(size_t)NLM*6 + s] = acc;
      if( k == 0 ) ocount[b*(size_t)NLM + l] = cnt;
    }
  }
  if( !( flags & RKFD_CF_F_GENF ) ) return;
  SYNC();

  /* 4. lane = coordinate: its owner and unit twist stay in registers */
  const bool con = lane < ND;
  const int own = con ? tj.cown[lane] : -1;
  double S[6], g = 0;
#pragma unroll
  for( int k=0; k<6; k++ ) S[k] = con ? SC[6*lane+k] : 0.0;
  for( int l=0; l<NLM; l++ ){
    if( CNT[l] == 0 ) continue;
    double E[9], col[6], lin[3], ang[3];
    bool hit;
    rkfd_jac_walk( tj, AE, AB, l, own, S, E, col, &hit );
    d_tmulv( E, col, lin ); d_tmulv( E, col+3, ang );
    if( hit ) g += lin[0]*WF[6*l] + lin[1]*WF[6*l+1] + lin[2]*WF[6*l+2] + ang[0]*WF[6*l+3] + ang[1]*WF[6*l+4] + ang[2]*WF[6*l+5];
  }
  if( con ) ogenf[b*(size_t)ND + lane] = g;
}

#endif /* RKFD_CF_H */
