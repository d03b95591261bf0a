/* rkfd_jac.h - task-space Jacobians (rkfdBatchUpdateJacobians): the map from the packed joint rates of one instance to the world
 * velocity of chosen SITES (a model link plus a point in its frame) and of the centre of mass of every chain.  One instance per
 * 64-lane wavefront; compiles for gfx950 (rkfd_capi_jac.hip) and under the lane emulator (tests/emu/rkfd_emu_jac.cpp).  Like the
 * read-out of rkfd_links.h it is no part of the step kernels: it reads dis and the model's tables, writes its own buffers, and
 * lives outside csrc/device/.
 *
 * It works in MODEL space - the model's links, parents, org frames and joint types as rkfdModel has them -, so neither the device's
 * merge of rigidly attached links nor the three device links of a spherical joint enter.
 *
 * J is the exact linear map of the model's own velocity recursion v_i = Ra_i' ( v_p + w_p x pa_i ) + joint velocity (rkfd_links.h):
 * the step from the parent's twist to the link's is ( v, w ) -> ( E v + B w, E w ) with E = Ra', B = Ra' C(pa), C(x) w = w x x, and
 * such maps compose exactly, ( E2 E1, E2 B1 + B2 E1 ), whatever the matrices are.  The textbook axis x ( p_site - p_joint ) on
 * composed world frames equals it only for exactly orthonormal frames, which frames read from a file with ten digits are not.
 *   1. lane = model link, 64 at a time: ( E_i, B_i ) of every link from dis, into LDS; the unit twists S_c of the link's own
 *      coordinates in the link's frame (revolute / prismatic: local z; float and spherical rates are given in the joint-origin
 *      frame, Rj' turns them into the link's, as the read-out does) into LDS, from where lane = coordinate c takes its own.
 *   2. per target link a walk from the target up to its chain root, the same for every lane, composing X = ( E, B ) from link k's
 *      frame to the target's.  When the walk stands on the link that owns lane c's coordinate the lane takes X S_c; lanes whose
 *      link is never passed keep an exact 0.  At the root E' is the target's world rotation (the transpose of a product is the
 *      product of the transposes in reverse, exactly).
 *   3. a site: the column moved to the site point, turned into the world, stored - c is the fastest index, so the 64 lanes store
 *      consecutive addresses.
 *   4. the COM of a chain: lane c sums m_i R_i ( Jv_i + Jw_i x com_i ) over the chain's links IN INDEX ORDER in its own registers
 *      and divides by the chain's mass: no cross-lane reduction, no atomics, the same bits every time.
 * A breakable float joint contributes its six columns whether it has broken or not, as in the read-out and the step's kinematics.
 *
 * Conventions of the results: J [nsite][6][ndof], rows 0-2 the world velocity of the site point per unit rate, rows 3-5 the world
 * angular velocity of its link; Jcom [nchain][3][ndof]; zeros for a chain without mass. */
#ifndef RKFD_JAC_H
#define RKFD_JAC_H

#include "rkfd_model.h"
#include "rkfd_devmodel.h"
#include "device/rkfd_dev_base.h"

#define RKFD_JAC_F_SITES 1
#define RKFD_JAC_F_COM   2
#define RKFD_JAC_MAX_SITES 64
#ifndef RKFD_LINKS_WAVES
#define RKFD_LINKS_WAVES 4      /* instances (wavefronts) of one workgroup: that of the read-out (rkfd_links.h) */
#endif

/* every pointer a device pointer (host under the emulator); all tables in MODEL space */
typedef struct {
  int nlink, nchain, ndof, nsite;
  const int *parent, *jtype, *dofoff;     /* [nlink] the model's */
  const double *org;                      /* [nlink*12] */
  const int *cown;                        /* [ndof] model link whose joint owns the coordinate */
  const int *chain_off, *chain_idx;       /* [nchain+1], [nlink]: the links of a chain, in index order */
  const int *site_link;                   /* [nsite] */
  const double *site_point;               /* [nsite*3] in the link's frame */
  const double *mass, *com;               /* [nlink], [nlink*3]; with a table of per-instance parameters the rows of */
  int par_stride;                         /* instance 0, par_stride doubles from one instance's row to the next (0: the model's, shared) */
} rkfdJacTab;

/* doubles of LDS one instance takes: ( E, B ) of every model link and the unit twists of the coordinates.  Lane = link writes them
 * with a stride of 9 doubles (18 banks: the 16 lanes an 8-byte store serves at once fall on 16 different bank pairs); the walks read
 * them at one address for all lanes, which the LDS broadcasts */
#define RKFD_JAC_LDS_DOUBLES(NLM, ND) ( 18*(NLM) + 6*(ND) )

/* the walk from model link `tgt` to its chain root: col = X( tgt <- owner of the lane's coordinate ) S (zero and hit = false when
 * the owner is no ancestor of tgt and not tgt itself), E = the transpose of tgt's world rotation.  Every lane walks the same links. */
RKFD_DEV void rkfd_jac_walk(const rkfdJacTab &t, const double *AE, const double *AB, int tgt, int own, const double *S, double *E, double *col, bool *hit)
{
  double B[9];
#pragma unroll
  for( int k=0; k<9; k++ ){ E[k] = ( k == 0 || k == 4 || k == 8 ) ? 1.0 : 0.0; B[k] = 0; }
#pragma unroll
  for( int k=0; k<6; k++ ) col[k] = 0;
  *hit = false;
  for( int l=tgt; l>=0; l=t.parent[l] ){
    if( own == l ){
      double u[3], w[3];
      d_mulv( E, S, u ); d_mulv( B, S+3, w );
      col[0] = u[0]+w[0]; col[1] = u[1]+w[1]; col[2] = u[2]+w[2];
      d_mulv( E, S+3, col+3 );
      *hit = true;
    }
    double El[9], Bl[9], M1[9], M2[9];
#pragma unroll
    for( int k=0; k<9; k++ ){ El[k] = AE[9*l+k]; Bl[k] = AB[9*l+k]; }
    /* X <- X o ( El, Bl ): ( E El, E Bl + B El ) */
    d_mul33( E, Bl, M1 ); d_mul33( B, El, M2 );
#pragma unroll
    for( int k=0; k<9; k++ ) B[k] = M1[k] + M2[k];
    d_mul33( E, El, E );
  }
}

RKFD_DEV void rkfd_jac_instance(const rkfdJacTab &t, const double *dis, size_t b, int lane, double *lds, int flags, double *oJ, double *oJcom)
{
  const int NLM = t.nlink, ND = t.ndof, NCH = t.nchain;
  double *AE = lds, *AB = AE + 9*NLM, *SC = AB + 9*NLM;
  const double *q = dis + b*ND;

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

  /* lane = coordinate: its owner and unit twist stay in registers */
  const bool con = lane < ND;
  const int own = con ? t.cown[lane] : -1;
  double S[6];
#pragma unroll
  for( int k=0; k<6; k++ ) S[k] = con ? SC[6*lane+k] : 0.0;

  /* 2. + 3. the sites */
  if( flags & RKFD_JAC_F_SITES ){
    for( int s=0; s<t.nsite; s++ ){
      const int tgt = t.site_link[s];
      const double pt[3] = { t.site_point[3*s], t.site_point[3*s+1], t.site_point[3*s+2] };
      double E[9], col[6], tt[3], lin[3], ang[3];
      bool hit;
      rkfd_jac_walk( t, AE, AB, tgt, own, S, E, col, &hit );
      d_cross( col+3, pt, tt );
      tt[0] += col[0]; tt[1] += col[1]; tt[2] += col[2];
      d_tmulv( E, tt, lin ); d_tmulv( E, col+3, ang );
      if( con ){
        double *dst = oJ + ( b*t.nsite + s )*6*(size_t)ND + lane;
#pragma unroll
        for( int k=0; k<3; k++ ){ dst[(size_t)k*ND] = hit ? lin[k] : 0.0; dst[(size_t)(3+k)*ND] = hit ? ang[k] : 0.0; }
      }
    }
  }

  /* 2. + 4. the centres of mass: the chain's links in index order, every lane its own sum */
  if( flags & RKFD_JAC_F_COM ){
    const size_t row = b*(size_t)t.par_stride;
    for( int c=0; c<NCH; c++ ){
      double acc[3] = { 0, 0, 0 }, M = 0;
      for( int x=t.chain_off[c]; x<t.chain_off[c+1]; x++ ){
        const int i = t.chain_idx[x];
        const double ms = t.mass[row+i];
        M += ms;
        if( ms != 0.0 ){
          const double cm[3] = { t.com[row+3*i], t.com[row+3*i+1], t.com[row+3*i+2] };
          double E[9], col[6], tt[3], vc[3];
          bool hit;
          rkfd_jac_walk( t, AE, AB, i, own, S, E, col, &hit );
          d_cross( col+3, cm, tt );
          tt[0] += col[0]; tt[1] += col[1]; tt[2] += col[2];
          d_tmulv( E, tt, vc );
          if( hit ){ acc[0] += ms*vc[0]; acc[1] += ms*vc[1]; acc[2] += ms*vc[2]; }
        }
      }
      if( con ){
        double *dst = oJcom + ( b*NCH + c )*3*(size_t)ND + lane;
#pragma unroll
        for( int k=0; k<3; k++ ) dst[(size_t)k*ND] = M > 0 ? acc[k]/M : 0.0;
      }
    }
  }
}

#endif /* RKFD_JAC_H */
