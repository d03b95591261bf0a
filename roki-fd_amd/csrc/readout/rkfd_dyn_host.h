/* rkfd_dyn_host.h - host side of the joint-space dynamics (rkfdBatchUpdateDynamics): the tables of rkfdDynTab that are not plain
 * copies of the model's arrays - the link that owns every joint coordinate, the children of every link and the links of every depth
 * level in index order, the mask of the coordinates on the way from a coordinate's owner to its root, the reflected rotor inertia of
 * the DC-motor joints, and mass | com | inertia in the row layout of a per-instance table (13 doubles per link).  Shared by
 * rkfd_capi_dyn.hip and the lane emulator's harness. */
#ifndef RKFD_DYN_HOST_H
#define RKFD_DYN_HOST_H

#include <vector>
#include <stdio.h>
#include <string.h>
#include "rkfd_model.h"

#define RKFD_DYN_HOST_LDS_MAX ( 160*1024 )      /* bytes of LDS one workgroup can have */

struct rkfdDynHostTab {
  int nlevel;
  std::vector<int> cown, lev_off, lev_idx, child_off, child_idx;
  std::vector<unsigned long long> amask;
  std::vector<double> rotor;
  std::vector<double> mci;      /* mass [nlink] | com [nlink*3] | inertia [nlink*9] */
};

/* (for a model of at most 64 joint coordinates: the masks are 64 bits) */
static inline void rkfd_dyn_host_build(const rkfdModel *m, rkfdDynHostTab *o)
{
  const int NLM = m->nlink, ND = m->ndof;
  const size_t nl1 = NLM > 0 ? NLM : 1, nd1 = ND > 0 ? ND : 1;
  o->cown.assign( nd1, 0 );
  o->rotor.assign( nd1, 0.0 );
  for( int i=0; i<NLM; i++ ){
    for( int k=0; k<rkfd_joint_dof( m->jtype[i] ); k++ ) o->cown[m->dofoff[i]+k] = i;
    if( ( m->jtype[i] == RKFD_JOINT_REVOL || m->jtype[i] == RKFD_JOINT_PRISM ) && m->mtype[i] == RKFD_MOTOR_DC )
      o->rotor[m->dofoff[i]] = m->mot_gear[i]*m->mot_gear[i]*m->mot_inertia[i];
  }
  /* depth levels and child lists: parent[i] < i, so one pass in index order gives both in index order */
  std::vector<int> depth( nl1, 0 );
  o->nlevel = 0;
  o->child_off.assign( NLM+1, 0 ); o->child_idx.assign( nl1, 0 );
  for( int i=0; i<NLM; i++ ){
    const int p = m->parent[i];
    depth[i] = p >= 0 ? depth[p]+1 : 0;
    if( depth[i]+1 > o->nlevel ) o->nlevel = depth[i]+1;
    if( p >= 0 ) o->child_off[p+1]++;
  }
  for( int i=0; i<NLM; i++ ) o->child_off[i+1] += o->child_off[i];
  o->lev_off.assign( o->nlevel+1, 0 ); o->lev_idx.assign( nl1, 0 );
  for( int i=0; i<NLM; i++ ) o->lev_off[depth[i]+1]++;
  for( int l=0; l<o->nlevel; l++ ) o->lev_off[l+1] += o->lev_off[l];
  {
    std::vector<int> cc( o->child_off.begin(), o->child_off.end()-1 ), lc( o->lev_off.begin(), o->lev_off.end()-1 );
    for( int i=0; i<NLM; i++ ){
      if( m->parent[i] >= 0 ) o->child_idx[cc[m->parent[i]]++] = i;
      o->lev_idx[lc[depth[i]]++] = i;
    }
  }
  /* bit a of amask[c]: coordinate a belongs to the joint of c's owner or of one of its ancestors */
  o->amask.assign( nd1, 0ull );
  {
    std::vector<unsigned long long> lm( nl1, 0ull );
    for( int i=0; i<NLM; i++ ){
      lm[i] = m->parent[i] >= 0 ? lm[m->parent[i]] : 0ull;
      for( int k=0; k<rkfd_joint_dof( m->jtype[i] ); k++ ) if( m->dofoff[i]+k < 64 ) lm[i] |= 1ull << ( m->dofoff[i]+k );
    }
    for( int c=0; c<ND; c++ ) o->amask[c] = lm[o->cown[c]];
  }
  o->mci.resize( (size_t)13*NLM + 1 );
  memcpy( o->mci.data(), m->mass, sizeof(double)*NLM );
  memcpy( o->mci.data() + NLM, m->com, sizeof(double)*3*NLM );
  memcpy( o->mci.data() + 4*(size_t)NLM, m->inertia, sizeof(double)*9*NLM );
}

/* the rows of a table of per-instance parameters, [batch][13 nlink]: mass | com | inertia of every instance */
static inline void rkfd_dyn_host_rows(int nlink, size_t batch, const double *par_mass, const double *par_com, const double *par_inertia, std::vector<double> *rows)
{
  const size_t NLM = nlink;
  rows->resize( batch*13*NLM + 1 );
  for( size_t i=0; i<batch; i++ ){
    double *r = rows->data() + i*13*NLM;
    memcpy( r, par_mass + i*NLM, sizeof(double)*NLM );
    memcpy( r + NLM, par_com + i*3*NLM, sizeof(double)*3*NLM );
    memcpy( r + 4*NLM, par_inertia + i*9*NLM, sizeof(double)*9*NLM );
  }
}

/* instances per workgroup by the LDS one instance needs: 4, else 2, else 1; 0 when one instance does not fit */
static inline int rkfd_dyn_host_waves(size_t lds_bytes_per_instance)
{
  for( int w=4; w>=1; w>>=1 ) if( lds_bytes_per_instance*w <= RKFD_DYN_HOST_LDS_MAX ) return w;
  return 0;
}

/* ---- rkfd_capi_dyn.hip: the joint-space dynamics of one batch (kernel, tables and result buffers on the batch's device), used by
 * rkfd_capi.hip's rkfdBatchUpdateDynamics / GetDynamics.  The caller has selected the device.  Failures return -1 (NULL) with a
 * message in err. */
struct rkfdDyn;
extern "C" rkfdDyn *rkfd_dyn_create(const rkfdModel *m, int batch, char *err, int errlen);
extern "C" void rkfd_dyn_destroy(rkfdDyn *d);
/* one launch on `stream` from the device arrays dis / vel [batch][ndof]; par_mass / par_com / par_inertia: the host copies of a table
 * of per-instance parameters in model space (all NULL: the model's), par_gen its generation */
extern "C" int rkfd_dyn_launch(rkfdDyn *d, const double *dis, const double *vel, int flags, const double *par_mass, const double *par_com,
                               const double *par_inertia, int par_gen, void *stream, char *err, int errlen);
/* flags of the last launch (0: none yet); host copies after waiting for it */
extern "C" int rkfd_dyn_flags(const rkfdDyn *d);
extern "C" int rkfd_dyn_get(rkfdDyn *d, double *M, double *h, double *g, char *err, int errlen);
/* which: 0 M, 1 h, 2 g; NULL before the first launch that needed it */
extern "C" const double *rkfd_dyn_dev(const rkfdDyn *d, int which);

#endif /* RKFD_DYN_HOST_H */
