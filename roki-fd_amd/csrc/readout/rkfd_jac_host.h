/* rkfd_jac_host.h - host side of the task-space Jacobians: the tables of rkfdJacTab that are not plain copies of the model's arrays
 * (the link that owns every joint coordinate, the chains' link lists, masses and centres of mass in the row layout of a per-instance
 * table), and the check of a list of sites.  Shared by rkfd_capi_jac.hip and the lane emulator's harness. */
#ifndef RKFD_JAC_HOST_H
#define RKFD_JAC_HOST_H

#include <vector>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "rkfd_model.h"

#define RKFD_JAC_HOST_MAX_SITES 64

struct rkfdJacHostTab {
  std::vector<int> cown, chain_off, chain_idx;
  std::vector<double> masscom;      /* mass [nlink] | com [nlink*3], the row layout of a per-instance table too */
};

static inline void rkfd_jac_host_build(const rkfdModel *m, rkfdJacHostTab *o)
{
  const int NLM = m->nlink, NCH = m->nchain;
  o->cown.assign( m->ndof > 0 ? m->ndof : 1, 0 );
  for( int i=0; i<NLM; i++ )
    for( int k=0; k<rkfd_joint_dof( m->jtype[i] ); k++ ) o->cown[m->dofoff[i]+k] = i;
  o->chain_off.assign( NCH+1, 0 ); o->chain_idx.assign( NLM > 0 ? NLM : 1, 0 );
  for( int i=0; i<NLM; i++ ) if( m->chain[i] >= 0 && m->chain[i] < NCH ) o->chain_off[m->chain[i]+1]++;
  for( int c=0; c<NCH; c++ ) o->chain_off[c+1] += o->chain_off[c];
  {
    std::vector<int> cur( o->chain_off.begin(), o->chain_off.end()-1 );
    for( int i=0; i<NLM; i++ ) if( m->chain[i] >= 0 && m->chain[i] < NCH ) o->chain_idx[cur[m->chain[i]]++] = i;
  }
  o->masscom.resize( (size_t)4*NLM + 1 );
  memcpy( o->masscom.data(), m->mass, sizeof(double)*NLM );
  memcpy( o->masscom.data() + NLM, m->com, sizeof(double)*3*NLM );
}

/* 0, or -1 with a message: a list of sites the Jacobians can take (point may be NULL: the link origins) */
static inline int rkfd_jac_check_sites(int nlink, int nsite, const int *link, const double *point, char *err, int errlen)
{
  if( nsite < 0 || nsite > RKFD_JAC_HOST_MAX_SITES ){ snprintf( err, errlen, "nsite must be within 0 .. %d (got %d)", RKFD_JAC_HOST_MAX_SITES, nsite ); return -1; }
  if( nsite > 0 && !link ){ snprintf( err, errlen, "null list of links" ); return -1; }
  for( int s=0; s<nsite; s++ ){
    if( link[s] < 0 || link[s] >= nlink ){ snprintf( err, errlen, "site %d: link %d is not within the model's 0 .. %d", s, link[s], nlink-1 ); return -1; }
    for( int k=0; point && k<3; k++ )
      if( !isfinite( point[3*s+k] ) ){ snprintf( err, errlen, "site %d: the point is not finite", s ); return -1; }
  }
  return 0;
}

/* ---- rkfd_capi_jac.hip: the Jacobians of one batch (kernel, tables, sites and result buffers on the batch's device), used by
 * rkfd_capi.hip's rkfdBatchSetJacobianSites / UpdateJacobians / GetJacobians.  The caller has selected the device.  Failures return
 * -1 (NULL) with a message in err. */
struct rkfdJac;
extern "C" rkfdJac *rkfd_jac_create(const rkfdModel *m, int batch, char *err, int errlen);
extern "C" void rkfd_jac_destroy(rkfdJac *j);
/* synchronous: waits for the last launch, then replaces the sites (the result buffer is reallocated only when nsite changes; a
 * refused list leaves the previous sites in place) */
extern "C" int rkfd_jac_set_sites(rkfdJac *j, int nsite, const int *link, const double *point, char *err, int errlen);
extern "C" int rkfd_jac_nsite(const rkfdJac *j);
/* one launch on `stream` from the device array dis [batch][ndof]; par_mass / par_com / par_gen as rkfd_links_launch takes them */
extern "C" int rkfd_jac_launch(rkfdJac *j, const double *dis, int flags, const double *par_mass, const double *par_com, int par_gen,
                               void *stream, char *err, int errlen);
/* flags of the last launch (0: none yet; replacing the sites takes RKFD_JAC_SITES out of them); host copies after waiting for it */
extern "C" int rkfd_jac_flags(const rkfdJac *j);
extern "C" int rkfd_jac_get(rkfdJac *j, double *J, double *Jcom, char *err, int errlen);
/* which: 0 J, 1 Jcom; NULL before the first launch that needed it */
extern "C" const double *rkfd_jac_dev(const rkfdJac *j, int which);

#endif /* RKFD_JAC_HOST_H */
