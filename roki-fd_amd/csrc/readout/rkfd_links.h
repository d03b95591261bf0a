/* rkfd_links.h - the task-space read-out (rkfdBatchUpdateLinks): poses and velocities of every MODEL link and the centre of mass
 * of every chain, from the packed joint state of one instance.  One instance per 64-lane wavefront; compiles for gfx950
 * (rkfd_capi_links.hip) and under the lane emulator (tests/emu/rkfd_emu_links.cpp).  It is no part of the step kernels: it reads
 * dis / vel and the world's tables, writes its own buffers, and lives outside csrc/device/ so that the step kernels, their
 * ahead-of-time code objects and their resource reports do not depend on it.
 *
 * The route is that of rkfd_phase_kinematics (device/rkfd_dev_kinematics.h): lane = device link, adjacent transform = org frame x
 * joint transform, pointer jumping over `anc` composes the world frames.  Differences: positions stay ABSOLUTE (the anchor link
 * is not subtracted); the velocities ride along in the same scan as LINK-FRAME twists (the recursion v_i = Ra_i' ( v_parent +
 * w_parent x pa_i ) + joint velocity, which is what is handed out, and which no far-away Pluecker origin enters); and the results
 * are per MODEL link: a rigidly attached link is its device link's frame composed with its frame in it, a spherical joint's link
 * is the last of its three device links.
 * A breakable float joint is a float joint here whether it has broken or not (rkfd_dev_brf.h: the link sits where its six
 * coordinates put it, its rates are what the state holds), so the broken flags are not read.
 *
 * Conventions of the results (DEVIATIONS.md item 1): R row-major, link -> world; p world; v = (linear, angular) of the link
 * origin in the link's own frame; com / comvel of a chain in the world frame, zeros for a chain without mass. */
#ifndef RKFD_LINKS_H
#define RKFD_LINKS_H

#include "rkfd_model.h"
#include "rkfd_devmodel.h"
#include "device/rkfd_dev_base.h"

#define RKFD_LINKS_F_POSE 1
#define RKFD_LINKS_F_VEL  2
#define RKFD_LINKS_F_COM  4
#define RKFD_LINKS_WAVES  4      /* instances (wavefronts) of one workgroup */

/* what the read-out needs besides the batch's device model: every pointer a device pointer (host under the emulator) */
typedef struct {
  int nlink, nlink_model, nchain, ndof, nround;
  const int *linfo, *anc;      /* the device model's own: [nlink] RKFD_LI_*, [nround][nlink] */
  const double *dorg;          /* [nlink*12] org frame of the device link's own model link (the identity for the second and third link of a spherical joint) */
  const double *dpre;          /* [nlink*21] in front of it: frame (12) and velocity block (9, see mvel) of the model parent in the device parent */
  const int *mdev;             /* [nlink_model] device link a model link is part of */
  const double *mframe;        /* [nlink_model*12] its frame in that device link (R row-major, p) */
  const double *mvel;          /* [nlink_model*9] B of its velocity in terms of the device link's: v = R' v_dev + B w_dev, w = R' w_dev */
  const int *chain_off, *chain_idx;   /* [nchain+1], [nlink_model]: the model links of a chain, in index order */
  const double *mass, *com;    /* model space [nlink_model], [nlink_model*3]; with a table of per-instance parameters the rows of */
  int par_stride;              /* instance 0, par_stride doubles from one instance's row to the next (0: the model's, shared) */
} rkfdLinksTab;

/* doubles of LDS one instance takes: world frames and velocities of the device links, one staged output array of 64 model
 * links, the COM terms of every model link and the chain sums */
#define RKFD_LINKS_LDS_DOUBLES(NL, NLM, NCH) ( 27*(NL) + 9*RKFD_WAVE + 7*(NLM) + 7*(NCH) )

/* one output array of a block of up to 64 model links, lane = link with W doubles each, through LDS so that consecutive lanes
 * store consecutive addresses */
template<int W> RKFD_DEV void rkfd_links_store(double *ST, const double *x, bool on, int lane, int n, double *dst)
{
  SYNC();
  if( on ){
#pragma unroll
    for( int k=0; k<W; k++ ) ST[W*lane+k] = x[k];
  }
  SYNC();
  for( int e=lane; e<W*n; e+=RKFD_WAVE ) dst[e] = ST[e];
}

RKFD_DEV void rkfd_links_instance(const rkfdLinksTab &t, const double *dis, const double *vel, size_t b, int lane, double *lds, int flags,
                                  double *oR, double *op, double *ov, double *ocom, double *ocomvel)
{
  const int NL = t.nlink, NLM = t.nlink_model, NCH = t.nchain;
  double *XA = lds, *XB = XA + 6*NL, *V = XB + 6*NL, *XV = V + 6*NL, *ST = XV + 9*NL, *CW = ST + 9*RKFD_WAVE, *CS = CW + 7*NLM;
  const bool want_v = ( flags & ( RKFD_LINKS_F_VEL | RKFD_LINKS_F_COM ) ) != 0;
  const bool on = lane < NL;
  const int i = on ? lane : 0;
  const int li = t.linfo[i];
  const int jt = on ? RKFD_LI_JT( li ) : RKFD_JOINT_FIXED;
  const int off = RKFD_LI_OFF( li );
  const double *q = dis + b*t.ndof, *qd = vel + b*t.ndof;
  double R[9], p[3], Bv[9] = { 0,0,0, 0,0,0, 0,0,0 }, Rj[9] = { 1,0,0, 0,1,0, 0,0,1 }, qd1 = 0, qdf[6] = { 0,0,0,0,0,0 };
  int anc[RKFD_MAX_ROUND];
#pragma unroll
  for( int r=0; r<RKFD_MAX_ROUND; r++ ) anc[r] = ( on && r < t.nround ) ? t.anc[r*NL+i] : -1;

  /* adjacent transform = org frame * joint transform (rkfd_phase_kinematics) */
  {
    double o[12];
#pragma unroll
    for( int k=0; k<12; k++ ) o[k] = t.dorg[12*i+k];
#pragma unroll
    for( int k=0; k<9; k++ ) R[k] = o[k];
    p[0] = o[9]; p[1] = o[10]; p[2] = o[11];
    if( jt == RKFD_JOINT_REVOL ){
      double s, c;
      d_sincos( q[off], &s, &c );
      const double Rz[9] = { c,-s,0, s,c,0, 0,0,1 };
      d_mul33( o, Rz, R );
      qd1 = qd[off];
    } else if( jt == RKFD_JOINT_PRISM ){
      const double q1 = q[off];
      p[0] += q1*o[2]; p[1] += q1*o[5]; p[2] += q1*o[8];
      qd1 = qd[off];
    } else if( jt == RKFD_JOINT_FLOAT ){
      double qq[6], tt[3];
#pragma unroll
      for( int k=0; k<6; k++ ){ qq[k] = q[off+k]; qdf[k] = qd[off+k]; }
      d_from_aa( qq+3, Rj );
      d_mul33( o, Rj, R );
      d_mulv( o, qq, tt );
      p[0] += tt[0]; p[1] += tt[1]; p[2] += tt[2];
    } else if( jt >= RKFD_DJT_SPHX ){
      /* spherical joint as three device links: the pseudo-links sit in the joint-origin frame, the real link (SPHZ, last
       * coordinate) is turned by the angle-axis vector of all three coordinates */
      qd1 = qd[off];
      if( jt == RKFD_DJT_SPHZ ){
        const double aa[3] = { q[off-2], q[off-1], q[off] };
        d_from_aa( aa, Rj );
        d_mul33( o, Rj, R );
      }
    }
  }
  /* The velocities obey v_i = Ra_i' ( v_parent + w_parent x pa_i ) + joint velocity, link by link of the MODEL.  That is a linear
   * map of the parent's twist, ( v, w ) -> ( E v + B w, E w ) with E = Ra', B w = Ra' ( w x pa ), and such maps compose exactly
   * (E2 E1, E2 B1 + B2 E1) whatever the matrices are - R' ( w x p ) for a composed ( R, p ) would equal it only for exactly
   * orthonormal frames, which frames read from a file with ten digits are not.  So the scan carries B beside ( R, p ); E is R'.
   * In front of the link's own joint sits the rigid chain from the device parent to the model parent (dpre, from the host). */
  {
    double T[12], Bp[9], Ra[9], pa[3], tt[3], C[9], M[9];
#pragma unroll
    for( int k=0; k<12; k++ ) T[k] = t.dpre[21*i+k];
#pragma unroll
    for( int k=0; k<9; k++ ){ Bp[k] = t.dpre[21*i+12+k]; Ra[k] = R[k]; }
    pa[0] = p[0]; pa[1] = p[1]; pa[2] = p[2];
    /* B = Ra' ( Bp + C(pa) T_R' ), C(pa) w = w x pa */
    const double Cx[9] = { 0, pa[2], -pa[1], -pa[2], 0, pa[0], pa[1], -pa[0], 0 };
    const double TRt[9] = { T[0],T[3],T[6], T[1],T[4],T[7], T[2],T[5],T[8] }, Rat[9] = { Ra[0],Ra[3],Ra[6], Ra[1],Ra[4],Ra[7], Ra[2],Ra[5],Ra[8] };
    d_mul33( Cx, TRt, C );
#pragma unroll
    for( int k=0; k<9; k++ ) M[k] = Bp[k] + C[k];
    d_mul33( Rat, M, Bv );
    d_mul33( T, Ra, R );
    d_mulv( T, pa, tt );
    p[0] = T[9]+tt[0]; p[1] = T[10]+tt[1]; p[2] = T[11]+tt[2];
  }
  /* the joint's own velocity, (linear, angular) in the link's frame: the rates of float and spherical joints are given in the
   * joint-origin frame, Rj' turns them into the link's */
  double v[6] = { 0,0,0,0,0,0 };
  if( want_v ){
    if( jt == RKFD_JOINT_REVOL ) v[5] = qd1;
    else if( jt == RKFD_JOINT_PRISM ) v[2] = qd1;
    else if( jt == RKFD_JOINT_FLOAT ){ d_tmulv( Rj, qdf, v ); d_tmulv( Rj, qdf+3, v+3 ); }
    else if( jt == RKFD_DJT_SPHX ) v[3] = qd1;
    else if( jt == RKFD_DJT_SPHY ) v[4] = qd1;
    else if( jt == RKFD_DJT_SPHZ ){ const double wz[3] = { 0, 0, qd1 }; d_tmulv( Rj, wz, v+3 ); }
  }
  if( on ){
#pragma unroll
    for( int k=0; k<6; k++ ){ XA[6*i+k] = R[k]; XB[6*i+k] = k < 3 ? R[6+k] : p[k-3]; V[6*i+k] = v[k]; }
#pragma unroll
    for( int k=0; k<9; k++ ) XV[9*i+k] = Bv[k];
  }
  SYNC();
  /* pointer jumping: compose with the ancestor 2^r levels up.  ( R, p, B ) is the link's frame and velocity map relative to the
   * frame the ancestor's own ( Ra, pa, Ba ) start from, v the link's velocity relative to that frame */
#pragma unroll
  for( int r=0; r<RKFD_MAX_ROUND; r++ ){
    if( r >= t.nround ) break;
    const int a = anc[r];
    if( a >= 0 ){
      double Ra[9], pa[3], tt[3];
#pragma unroll
      for( int k=0; k<6; k++ ) Ra[k] = XA[6*a+k];
#pragma unroll
      for( int k=0; k<3; k++ ){ Ra[6+k] = XB[6*a+k]; pa[k] = XB[6*a+3+k]; }
      if( want_v ){
        double va[6], u[3], Ba[9], M1[9], M2[9];
#pragma unroll
        for( int k=0; k<6; k++ ) va[k] = V[6*a+k];
#pragma unroll
        for( int k=0; k<9; k++ ) Ba[k] = XV[9*a+k];
        /* v += E va + B wa, w += E wa; then B = E Ba + B Ea  (E = R', Ea = Ra') */
        d_tmulv( R, va, u ); d_mulv( Bv, va+3, tt );
        v[0] += u[0]+tt[0]; v[1] += u[1]+tt[1]; v[2] += u[2]+tt[2];
        d_tmulv( R, va+3, u );
        v[3] += u[0]; v[4] += u[1]; v[5] += u[2];
        const double Rt[9] = { R[0],R[3],R[6], R[1],R[4],R[7], R[2],R[5],R[8] }, Rat[9] = { Ra[0],Ra[3],Ra[6], Ra[1],Ra[4],Ra[7], Ra[2],Ra[5],Ra[8] };
        d_mul33( Rt, Ba, M1 ); d_mul33( Bv, Rat, M2 );
#pragma unroll
        for( int k=0; k<9; k++ ) Bv[k] = M1[k] + M2[k];
      }
      d_mulv( Ra, p, tt );
      p[0] = pa[0]+tt[0]; p[1] = pa[1]+tt[1]; p[2] = pa[2]+tt[2];
      d_mul33( Ra, R, R );
    }
    SYNC();
    if( a >= 0 ){
#pragma unroll
      for( int k=0; k<6; k++ ){ XA[6*i+k] = R[k]; XB[6*i+k] = k < 3 ? R[6+k] : p[k-3]; V[6*i+k] = v[k]; }
#pragma unroll
      for( int k=0; k<9; k++ ) XV[9*i+k] = Bv[k];
    }
    SYNC();
  }

  /* lane = model link, 64 at a time: its frame in the device link's, the device link's twist moved to its origin and turned
   * into its frame */
  for( int j0=0; j0<NLM; j0+=RKFD_WAVE ){
    const int j = j0 + lane, n = NLM - j0 < RKFD_WAVE ? NLM - j0 : RKFD_WAVE;
    const bool mon = j < NLM;
    const int jj = mon ? j : 0;
    const int r = t.mdev[jj];
    double Rr[9], pr[3], T[12], Rm[9], pm[3], vm[6] = { 0,0,0,0,0,0 }, tt[3];
#pragma unroll
    for( int k=0; k<6; k++ ) Rr[k] = XA[6*r+k];
#pragma unroll
    for( int k=0; k<3; k++ ){ Rr[6+k] = XB[6*r+k]; pr[k] = XB[6*r+3+k]; }
#pragma unroll
    for( int k=0; k<12; k++ ) T[k] = t.mframe[12*jj+k];
    d_mul33( Rr, T, Rm );
    d_mulv( Rr, T+9, tt );
    pm[0] = pr[0]+tt[0]; pm[1] = pr[1]+tt[1]; pm[2] = pr[2]+tt[2];
    if( want_v ){
      /* the device link's velocity moved to the model link's origin and turned into its frame */
      double vr[6], Bm[9];
#pragma unroll
      for( int k=0; k<6; k++ ) vr[k] = V[6*r+k];
#pragma unroll
      for( int k=0; k<9; k++ ) Bm[k] = t.mvel[9*jj+k];
      d_tmulv( T, vr, vm ); d_mulv( Bm, vr+3, tt );
      vm[0] += tt[0]; vm[1] += tt[1]; vm[2] += tt[2];
      d_tmulv( T, vr+3, vm+3 );
    }
    const size_t base = b*NLM + j0;
    if( flags & RKFD_LINKS_F_POSE ){
      rkfd_links_store<9>( ST, Rm, mon, lane, n, oR + 9*base );
      rkfd_links_store<3>( ST, pm, mon, lane, n, op + 3*base );
    }
    if( flags & RKFD_LINKS_F_VEL ) rkfd_links_store<6>( ST, vm, mon, lane, n, ov + 6*base );
    if( ( flags & RKFD_LINKS_F_COM ) && mon ){
      /* m, m ( p + R c ), m R ( v + w x c ) */
      const size_t row = b*(size_t)t.par_stride;
      const double ms = t.mass[row+j], c[3] = { t.com[row+3*j], t.com[row+3*j+1], t.com[row+3*j+2] };
      double cw[3], vc[3];
      d_mulv( Rm, c, cw );
      d_cross( vm+3, c, tt );
      tt[0] += vm[0]; tt[1] += vm[1]; tt[2] += vm[2];
      d_mulv( Rm, tt, vc );
      CW[7*j] = ms;
#pragma unroll
      for( int k=0; k<3; k++ ){ CW[7*j+1+k] = ms*( pm[k]+cw[k] ); CW[7*j+4+k] = ms*vc[k]; }
    }
  }
  if( flags & RKFD_LINKS_F_COM ){
    SYNC();
    /* one lane per ( chain, term ): the sum over the chain's links in index order */
    for( int e=lane; e<7*NCH; e+=RKFD_WAVE ){
      const int c = e/7, k = e - 7*c;
      double s = 0;
      for( int x=t.chain_off[c]; x<t.chain_off[c+1]; x++ ) s += CW[7*t.chain_idx[x]+k];
      CS[e] = s;
    }
    SYNC();
    for( int e=lane; e<3*NCH; e+=RKFD_WAVE ){
      const int c = e/3, k = e - 3*c;
      const double M = CS[7*c];
      ocom[b*3*NCH+e] = M > 0 ? CS[7*c+1+k]/M : 0.0;
      ocomvel[b*3*NCH+e] = M > 0 ? CS[7*c+4+k]/M : 0.0;
    }
  }
}

#endif /* RKFD_LINKS_H */
