/* rkfd_dyn.h - joint-space dynamics (rkfdBatchUpdateDynamics): the joint-space inertia matrix M, the bias force h = rnea( q, qd, 0 )
 * and the gravity force g = rnea( q, 0, 0 ) of one instance, from its live dis / vel:  M qdd + h = generalised force.  One instance
 * per 64-lane wavefront; compiles for gfx950 (rkfd_capi_dyn.hip) and under the lane emulator (tests/emu/rkfd_emu_dyn.cpp).  Like the
 * read-out and the Jacobians it is no part of the step kernels: it reads dis / vel and the model's tables, writes its own buffers, and
 * lives outside csrc/device/.
 *
 * It works in MODEL space, in every link's OWN frame about the link's origin, with the exact linear map of the model's velocity
 * recursion (rkfd_jac.h): the twist of link i is X_i = ( E, B ) = ( Ra', Ra' C(pa) ) applied to its parent's, plus S_c rate_c of its
 * own coordinates.  Then 0.5 vel' M vel is the kinetic energy sum_i 0.5 m_i | v_i + w_i x c_i |^2 + 0.5 w_i' I_i w_i of exactly the
 * velocities the read-out reports, whatever the frames of the file are: the composite inertia of a subtree is carried as a general
 * symmetric 6 x 6 matrix (21 numbers), Ic_p += X_i' Ic_i X_i, because X' Ic X keeps the ten-number rigid-body form only for exactly
 * orthonormal frames, which frames read from a file with ten digits are not.
 *   1. lane = model link, 64 at a time: ( E_i, B_i ) from dis and the unit twists S_c of the link's coordinates into LDS (as phase 1
 *      of rkfd_jac_instance).
 *   2. down the tree level by level (host-built level lists), the parent's values from LDS: angular velocity, angular acceleration
 *      and the acceleration of the link origin at qdd = 0 with the root's parent accelerating at +G z (classical Newton-Euler in the
 *      link's frame), and the same with vel = 0 (gravity alone).
 *   3. up the tree level by level: the lane of a link builds the link's own 6 x 6 inertia and wrenches and adds its children's,
 *      Ic += X' Ic_child X, f += X' f_child, IN INDEX ORDER from the host-built child list: a parent reads, sibling lanes never add
 *      into one address.
 *   4. lane = coordinate c.  For every row r, the same for all lanes: F = Ic_owner(r) S_r, carried from owner(r) to the root with X';
 *      when the walk stands on the link that owns lane c's coordinate the lane takes S_c' F = M[r][c].  Inside the block of one
 *      joint only c <= r is computed.  The lane stores M[r][c] and its mirror M[c][r] - the same bits -, or an exact 0.0 where
 *      neither owner is the other's ancestor (a host-built mask of the ancestors' coordinates decides, not the arithmetic); every
 *      element is written exactly once, by one lane.  h[c] = S_c' f_owner(c), g[c] likewise.
 * No atomics, no cross-lane reduction: the same bits every launch.
 *
 * Conventions of the results: M [ndof][ndof] with respect to the packed RATES (the columns of J); h, g [ndof] on the same
 * coordinates: revolute / prismatic the scalar about / along local z, float and breakable float (force, moment about the link origin)
 * on the joint-origin axes, spherical the moment on those axes.  A breakable float joint is a float joint whether broken or not.
 * Joint friction, actuator torques and contact forces are no part of h. */
#ifndef RKFD_DYN_H
#define RKFD_DYN_H

#include "rkfd_model.h"
#include "rkfd_devmodel.h"
#include "device/rkfd_dev_base.h"

#define RKFD_DYN_F_MASS    1
#define RKFD_DYN_F_BIAS    2
#define RKFD_DYN_F_GRAVITY 4
#define RKFD_DYN_F_ROTOR   8
#define RKFD_DYN_MAX_WAVES 4      /* instances (wavefronts) of one workgroup, at most: 4, 2 or 1 by the LDS one instance needs */

/* every pointer a device pointer (host under the emulator); all tables in MODEL space */
typedef struct {
  int nlink, ndof, nlevel;
  const int *parent, *jtype, *dofoff;     /* [nlink] the model's */
  const double *org;                      /* [nlink*12] */
  const int *cown;                        /* [ndof] model link whose joint owns the coordinate */
  const int *lev_off, *lev_idx;           /* [nlevel+1], [nlink]: the links of a depth level, in index order */
  const int *child_off, *child_idx;       /* [nlink+1], [nlink]: the children of a link, in index order */
  const unsigned long long *amask;        /* [ndof] bit a: coordinate a belongs to the owner of the coordinate or to an ancestor of it */
  const double *rotor;                    /* [ndof] gear^2 x rotor inertia of a DC-motor joint, 0 elsewhere */
  const double *mass, *com, *inertia;     /* [nlink], [nlink*3], [nlink*9]; with a table of per-instance parameters the rows of */
  int par_stride;                         /* instance 0, par_stride doubles from one instance's row to the next (0: the model's, shared) */
} rkfdDynTab;

/* doubles of LDS one instance takes: ( E, B ) of every model link (18), the unit twists of the coordinates (6 each), per link the
 * twelve numbers of phase 2 that phase 3 replaces by the two wrenches, and the composite inertia (21) */
#define RKFD_DYN_LDS_DOUBLES(NLM, ND) ( 51*(NLM) + 6*(ND) )

/* c = a' b */
RKFD_DEV void dyn_tmul33(const double *a, const double *b, double *c)
{
#pragma unroll
  for( int i=0; i<3; i++ )
#pragma unroll
    for( int j=0; j<3; j++ ) c[3*i+j] = a[i]*b[j] + a[3+i]*b[3+j] + a[6+i]*b[6+j];
}
/* a symmetric 6 x 6 matrix [[A, H], [H', D]] in 21 doubles: the upper triangle of A, H, the upper triangle of D */
RKFD_DEV void dyn_sym_store(double *p, const double *A, const double *H, const double *D)
{
  p[0] = A[0]; p[1] = A[1]; p[2] = A[2]; p[3] = A[4]; p[4] = A[5]; p[5] = A[8];
#pragma unroll
  for( int k=0; k<9; k++ ) p[6+k] = H[k];
  p[15] = D[0]; p[16] = D[1]; p[17] = D[2]; p[18] = D[4]; p[19] = D[5]; p[20] = D[8];
}
RKFD_DEV void dyn_sym_load(const double *p, double *A, double *H, double *D)
{
  A[0] = p[0]; A[1] = A[3] = p[1]; A[2] = A[6] = p[2]; A[4] = p[3]; A[5] = A[7] = p[4]; A[8] = p[5];
#pragma unroll
  for( int k=0; k<9; k++ ) H[k] = p[6+k];
  D[0] = p[15]; D[1] = D[3] = p[16]; D[2] = D[6] = p[17]; D[4] = p[18]; D[5] = D[7] = p[19]; D[8] = p[20];
}

RKFD_DEV void rkfd_dyn_instance(const rkfdDynTab &t, const double *dis, const double *vel, size_t b, int lane, double *lds, int flags,
                                double *oM, double *oh, double *og)
{
  const int NLM = t.nlink, ND = t.ndof, NLV = t.nlevel;
  double *AE = lds, *AB = AE + 9*NLM, *SC = AB + 9*NLM, *K = SC + 6*ND, *IC = K + 12*NLM;
  const double *q = dis + b*ND, *qd = vel + b*ND;
  const size_t row = b*(size_t)t.par_stride;
  const bool want_m = ( flags & RKFD_DYN_F_MASS ) != 0, want_f = ( flags & ( RKFD_DYN_F_BIAS | RKFD_DYN_F_GRAVITY ) ) != 0;

  /* 1. lane = model link: the adjacent map ( E, B ) = ( Ra', Ra' C(pa) ), Ra = org frame x joint transform, and the unit twists */
  for( int j0=0; j0<NLM; j0+=RKFD_WAVE ){
    const int j = j0 + lane;
    const bool on = j < NLM;
    const int jj = on ? j : 0;
    const int jt = on ? t.jtype[jj] : RKFD_JOINT_FIXED;
    const int off = t.dofoff[jj];
    double o[12], Ra[9], pa[3], Rj[9] = { 1,0,0, 0,1,0, 0,0,1 };
#pragma unroll
    for( int k=0; k<12; k++ ) o[k] = t.org[12*jj+k];
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

  /* 2. down the tree: K[12 i ..] = angular velocity w, angular acceleration al and acceleration a of the link origin at qdd = 0, and
   * the acceleration ag with vel = 0 as well, all in the link's frame.  The root's parent stands still and accelerates at +G z */
  if( want_f ){
    for( int L=0; L<NLV; L++ ){
      for( int x=t.lev_off[L]+lane; x<t.lev_off[L+1]; x+=RKFD_WAVE ){
        const int i = t.lev_idx[x], p = t.parent[i], off = t.dofoff[i];
        const int jt = t.jtype[i];
        const int nd = ( jt == RKFD_JOINT_FLOAT || jt == RKFD_JOINT_BRFLOAT ) ? 6 : ( jt == RKFD_JOINT_SPHER ? 3 : ( jt == RKFD_JOINT_FIXED ? 0 : 1 ) );
        double E[9], Bm[9], wp[3] = { 0,0,0 }, alp[3] = { 0,0,0 }, ap[3] = { 0,0,RKFD_G }, agp[3] = { 0,0,RKFD_G };
#pragma unroll
        for( int k=0; k<9; k++ ){ E[k] = AE[9*i+k]; Bm[k] = AB[9*i+k]; }
        if( p >= 0 ){
#pragma unroll
          for( int k=0; k<3; k++ ){ wp[k] = K[12*p+k]; alp[k] = K[12*p+3+k]; ap[k] = K[12*p+6+k]; agp[k] = K[12*p+9+k]; }
        }
        /* the joint's own velocity in the link's frame: sum S_c rate_c */
        double vJ[3] = { 0,0,0 }, wJ[3] = { 0,0,0 };
#pragma unroll
        for( int k=0; k<6; k++ )
          if( k < nd ){
            const double r = qd[off+k];
#pragma unroll
            for( int x=0; x<3; x++ ){ vJ[x] += SC[6*(off+k)+x]*r; wJ[x] += SC[6*(off+k)+3+x]*r; }
          }
        double Ew[3], w[3], al[3], a[3], ag[3], u[3], tt[3];
        d_mulv( E, wp, Ew );
        /* al = E al_p + ( E w_p ) x wJ */
        d_mulv( E, alp, al ); d_cross( Ew, wJ, tt );
#pragma unroll
        for( int k=0; k<3; k++ ){ w[k] = Ew[k] + wJ[k]; al[k] += tt[k]; }
        /* a = E ( a_p + al_p x pa + w_p x ( w_p x pa ) ) + 2 ( E w_p ) x vJ;  E ( x x pa ) = B x */
        d_mulv( E, ap, a ); d_mulv( Bm, alp, tt );
        a[0] += tt[0]; a[1] += tt[1]; a[2] += tt[2];
        d_mulv( Bm, wp, u ); d_cross( Ew, u, tt );
        a[0] += tt[0]; a[1] += tt[1]; a[2] += tt[2];
        d_cross( Ew, vJ, tt );
        a[0] += 2*tt[0]; a[1] += 2*tt[1]; a[2] += 2*tt[2];
        d_mulv( E, agp, ag );
#pragma unroll
        for( int k=0; k<3; k++ ){ K[12*i+k] = w[k]; K[12*i+3+k] = al[k]; K[12*i+6+k] = a[k]; K[12*i+9+k] = ag[k]; }
      }
      SYNC();
    }
  }

  /* 3. up the tree: the link's own inertia about its origin, [[ m 1, m C ], [ m C', I + m C'C ]] with C w = w x c, and its wrenches
   * ( f, n about the origin ) for the bias and for gravity alone, then the children's in index order */
  for( int L=NLV-1; L>=0; L-- ){
    for( int x=t.lev_off[L]+lane; x<t.lev_off[L+1]; x+=RKFD_WAVE ){
      const int i = t.lev_idx[x];
      const double ms = t.mass[row+i];
      const double c[3] = { t.com[row+3*i], t.com[row+3*i+1], t.com[row+3*i+2] };
      double In[9], A[9], H[9], D[9], fb[6] = { 0,0,0,0,0,0 }, fg[6] = { 0,0,0,0,0,0 };
#pragma unroll
      for( int k=0; k<9; k++ ) In[k] = t.inertia[row+9*i+k];
      if( want_m ){
        const double C[9] = { 0, c[2], -c[1], -c[2], 0, c[0], c[1], -c[0], 0 };
        const double cc = c[0]*c[0] + c[1]*c[1] + c[2]*c[2];
#pragma unroll
        for( int r=0; r<3; r++ )
#pragma unroll
          for( int s=0; s<3; s++ ){
            A[3*r+s] = r == s ? ms : 0.0;
            H[3*r+s] = ms*C[3*r+s];
            /* (the symmetric part of the inertia: the upper triangle is computed, the lower mirrors it) */
            D[3*r+s] = 0.5*( In[3*r+s] + In[3*s+r] ) + ms*( ( r == s ? cc : 0.0 ) - c[r]*c[s] );
          }
      }
      if( want_f ){
        double w[3], al[3], a[3], ag[3], tt[3], u[3], F[3], N[3];
#pragma unroll
        for( int k=0; k<3; k++ ){ w[k] = K[12*i+k]; al[k] = K[12*i+3+k]; a[k] = K[12*i+6+k]; ag[k] = K[12*i+9+k]; }
        /* F = m ( a + al x c + w x ( w x c ) ),  N = I al + w x I w,  n = N + c x F */
        d_cross( al, c, tt ); d_cross( w, c, u );
        a[0] += tt[0]; a[1] += tt[1]; a[2] += tt[2];
        d_cross( w, u, tt );
#pragma unroll
        for( int k=0; k<3; k++ ) F[k] = ms*( a[k] + tt[k] );
        d_mulv( In, w, u ); d_cross( w, u, tt ); d_mulv( In, al, N );
        d_cross( c, F, u );
#pragma unroll
        for( int k=0; k<3; k++ ){ fb[k] = F[k]; fb[3+k] = N[k] + tt[k] + u[k]; F[k] = ms*ag[k]; }
        d_cross( c, F, u );
#pragma unroll
        for( int k=0; k<3; k++ ){ fg[k] = F[k]; fg[3+k] = u[k]; }
      }
      for( int y=t.child_off[i]; y<t.child_off[i+1]; y++ ){
        const int ch = t.child_idx[y];
        double E[9], Bm[9];
#pragma unroll
        for( int k=0; k<9; k++ ){ E[k] = AE[9*ch+k]; Bm[k] = AB[9*ch+k]; }
        if( want_m ){
          /* X' Ic X, X = [[ E, B ], [ 0, E ]]: the diagonal blocks from their upper triangles */
          double Ac[9], Hc[9], Dc[9], T1[9], T2[9], Y01[9], Y11[9], Z[9], Z2[9];
          dyn_sym_load( IC + 21*ch, Ac, Hc, Dc );
          d_mul33( Ac, Bm, T1 ); d_mul33( Hc, E, T2 );
#pragma unroll
          for( int k=0; k<9; k++ ) Y01[k] = T1[k] + T2[k];
          dyn_tmul33( Hc, Bm, T1 ); d_mul33( Dc, E, T2 );
#pragma unroll
          for( int k=0; k<9; k++ ) Y11[k] = T1[k] + T2[k];
          d_mul33( Ac, E, T1 ); dyn_tmul33( E, T1, Z );
          A[0] += Z[0]; A[1] += Z[1]; A[2] += Z[2]; A[4] += Z[4]; A[5] += Z[5]; A[8] += Z[8];
          dyn_tmul33( E, Y01, Z );
#pragma unroll
          for( int k=0; k<9; k++ ) H[k] += Z[k];
          dyn_tmul33( Bm, Y01, Z ); dyn_tmul33( E, Y11, Z2 );
          D[0] += Z[0]+Z2[0]; D[1] += Z[1]+Z2[1]; D[2] += Z[2]+Z2[2]; D[4] += Z[4]+Z2[4]; D[5] += Z[5]+Z2[5]; D[8] += Z[8]+Z2[8];
        }
        if( want_f ){
          /* X' ( f, n ) = ( E' f, E' n + B' f ) */
          double fc[6], gc[6], tt[3], u[3];
#pragma unroll
          for( int k=0; k<6; k++ ){ fc[k] = K[12*ch+k]; gc[k] = K[12*ch+6+k]; }
          d_tmulv( E, fc, tt );
          fb[0] += tt[0]; fb[1] += tt[1]; fb[2] += tt[2];
          d_tmulv( E, fc+3, tt ); d_tmulv( Bm, fc, u );
          fb[3] += tt[0]+u[0]; fb[4] += tt[1]+u[1]; fb[5] += tt[2]+u[2];
          d_tmulv( E, gc, tt );
          fg[0] += tt[0]; fg[1] += tt[1]; fg[2] += tt[2];
          d_tmulv( E, gc+3, tt ); d_tmulv( Bm, gc, u );
          fg[3] += tt[0]+u[0]; fg[4] += tt[1]+u[1]; fg[5] += tt[2]+u[2];
        }
      }
      if( want_m ) dyn_sym_store( IC + 21*i, A, H, D );
      if( want_f ){
#pragma unroll
        for( int k=0; k<6; k++ ){ K[12*i+k] = fb[k]; K[12*i+6+k] = fg[k]; }
      }
    }
    SYNC();
  }

  /* 4. lane = coordinate */
  const bool con = lane < ND;
  const int cc = con ? lane : 0;
  const int own = con ? t.cown[cc] : -1;
  double S[6];
#pragma unroll
  for( int k=0; k<6; k++ ) S[k] = con ? SC[6*cc+k] : 0.0;
  if( want_f && con ){
    double hb = 0, hg = 0;
#pragma unroll
    for( int k=0; k<6; k++ ){ hb += S[k]*K[12*own+k]; hg += S[k]*K[12*own+6+k]; }
    if( flags & RKFD_DYN_F_BIAS ) oh[b*ND + lane] = hb;
    if( flags & RKFD_DYN_F_GRAVITY ) og[b*ND + lane] = hg;
  }
  if( want_m ){
    const unsigned long long mc = con ? t.amask[cc] : 0ull;
    const double rot = ( con && ( flags & RKFD_DYN_F_ROTOR ) ) ? t.rotor[cc] : 0.0;
    double *Mb = oM + b*(size_t)ND*ND;
    for( int r=0; r<ND; r++ ){
      const int ownr = t.cown[r];
      const unsigned long long mr = t.amask[r];
      /* F = Ic_owner(r) S_r: one address for all lanes */
      double A[9], H[9], D[9], Sr[6], F[6], tt[3], u[3], val = 0;
      dyn_sym_load( IC + 21*ownr, A, H, D );
#pragma unroll
      for( int k=0; k<6; k++ ) Sr[k] = SC[6*r+k];
      d_mulv( A, Sr, tt ); d_mulv( H, Sr+3, u );
      F[0] = tt[0]+u[0]; F[1] = tt[1]+u[1]; F[2] = tt[2]+u[2];
      d_tmulv( H, Sr, tt ); d_mulv( D, Sr+3, u );
      F[3] = tt[0]+u[0]; F[4] = tt[1]+u[1]; F[5] = tt[2]+u[2];
      for( int l=ownr; l>=0; l=t.parent[l] ){
        if( own == l ) val = S[0]*F[0] + S[1]*F[1] + S[2]*F[2] + S[3]*F[3] + S[4]*F[4] + S[5]*F[5];
        double E[9], Bm[9];
#pragma unroll
        for( int k=0; k<9; k++ ){ E[k] = AE[9*l+k]; Bm[k] = AB[9*l+k]; }
        d_tmulv( E, F+3, tt ); d_tmulv( Bm, F, u );
        F[3] = tt[0]+u[0]; F[4] = tt[1]+u[1]; F[5] = tt[2]+u[2];
        d_tmulv( E, F, tt );
        F[0] = tt[0]; F[1] = tt[1]; F[2] = tt[2];
      }
      if( con ){
        const bool in_r = ( mr >> lane ) & 1ull, in_c = ( mc >> r ) & 1ull;
        if( in_r && ( !in_c || lane <= r ) ){
          /* the coordinate of an ancestor's joint, or of the same joint and not above r: this lane's to compute, and to mirror */
          if( lane == r ) val += rot;
          Mb[(size_t)r*ND + lane] = val;
          if( lane != r ) Mb[(size_t)lane*ND + r] = val;
        } else if( !in_r && !in_c ) Mb[(size_t)r*ND + lane] = 0.0;
        /* (else: the mirror of what lane r stores in row `lane`) */
      }
    }
  }
}

#endif /* RKFD_DYN_H */
