/* rkfd_cf_host.h - host side of the contact read-out (rkfdBatchUpdateContactForces): the tables of rkfdCfTab that are not plain
 * copies of the model's arrays - the link that owns every joint coordinate, per candidate contact vertex the link that owns the
 * vertex, the other link of its pair and the vertex in the owner's frame (from cand_pair -> pair_shape -> shape_link, cand_side and
 * cand_vert -> verts), and per link the list of ( candidate, side ) in candidate index order.  Shared by rkfd_capi_cf.hip and the
 * lane emulator's harness, which may also hand in candidate tables of its own. */
#ifndef RKFD_CF_HOST_H
#define RKFD_CF_HOST_H

#include <vector>
#include <stdio.h>
#include <string.h>
#include "rkfd_model.h"

#define RKFD_CF_HOST_LDS_MAX ( 160*1024 )      /* bytes of LDS one workgroup can have */

struct rkfdCfHostTab {
  int ncand;
  std::vector<int> cown;              /* [ndof] */
  std::vector<int> c_own, c_oth;      /* [ncand] */
  std::vector<double> c_vert;         /* [ncand*3] */
  std::vector<int> l_off, l_ent;      /* [nlink+1], [2 ncand]: 2 x candidate + ( 1: the link is the other side of the pair ) */
};

/* own == NULL: the model's candidates; else ncand candidates given as owner link, other link and vertex in the owner's frame.
 * -1 with a message when a link index is out of range */
static inline int rkfd_cf_host_build(const rkfdModel *m, int ncand, const int *own, const int *oth, const double *vert, rkfdCfHostTab *o, char *err, int errlen)
{
  const int NLM = m->nlink, ND = m->ndof;
  o->cown.assign( ND > 0 ? ND : 1, 0 );
  for( int i=0; i<NLM; i++ )
    for( int k=0; k<rkfd_joint_dof( m->jtype[i] ); k++ ) o->cown[m->dofoff[i]+k] = i;
  const int NC = own ? ncand : m->ncand;
  o->ncand = NC;
  o->c_own.assign( NC > 0 ? NC : 1, 0 ); o->c_oth.assign( NC > 0 ? NC : 1, 0 ); o->c_vert.assign( NC > 0 ? 3*(size_t)NC : 1, 0.0 );
  for( int j=0; j<NC; j++ ){
    if( own ){
      o->c_own[j] = own[j]; o->c_oth[j] = oth[j];
      for( int k=0; k<3; k++ ) o->c_vert[3*j+k] = vert[3*j+k];
    } else {
      const int pr = m->cand_pair[j], sd = m->cand_side[j];
      o->c_own[j] = m->shape_link[m->pair_shape[2*pr + sd]];
      o->c_oth[j] = m->shape_link[m->pair_shape[2*pr + 1 - sd]];
      for( int k=0; k<3; k++ ) o->c_vert[3*j+k] = m->verts[3*(size_t)m->cand_vert[j]+k];
    }
    if( o->c_own[j] < 0 || o->c_own[j] >= NLM || o->c_oth[j] < 0 || o->c_oth[j] >= NLM ){
      if( err ) snprintf( err, errlen, "candidate %d names link %d / %d of %d", j, o->c_own[j], o->c_oth[j], NLM );
      return -1;
    }
  }
  /* per link, the candidates that touch it on either side: one pass in candidate order keeps every list in candidate order */
  o->l_off.assign( NLM+1, 0 ); o->l_ent.assign( NC > 0 ? 2*(size_t)NC : 1, 0 );
  for( int j=0; j<NC; j++ ){ o->l_off[o->c_own[j]+1]++; o->l_off[o->c_oth[j]+1]++; }
  for( int i=0; i<NLM; i++ ) o->l_off[i+1] += o->l_off[i];
  std::vector<int> at( o->l_off.begin(), o->l_off.end()-1 );
  for( int j=0; j<NC; j++ ){ o->l_ent[at[o->c_own[j]]++] = 2*j; o->l_ent[at[o->c_oth[j]]++] = 2*j+1; }
  return 0;
}

/* instances per workgroup by the LDS one instance needs: 4, else 2, else 1; 0 when one instance does not fit */
static inline int rkfd_cf_host_waves(size_t lds_bytes_per_instance)
{
  for( int w=4; w>=1; w>>=1 ) if( lds_bytes_per_instance*w <= RKFD_CF_HOST_LDS_MAX ) return w;
  return 0;
}

/* ---- rkfd_capi_cf.hip: the contact read-out of one batch (kernel, tables and result buffers on the batch's device), used by
 * rkfd_capi.hip's rkfdBatchUpdateContactForces[Dev] / GetContactForces.  The caller has selected the device.  Failures return -1
 * (NULL) with a message in err. */
struct rkfdCf;
extern "C" rkfdCf *rkfd_cf_create(const rkfdModel *m, int batch, char *err, int errlen);
extern "C" void rkfd_cf_destroy(rkfdCf *c);
/* one launch on `stream` from the device arrays dis [batch][ndof], active [batch][ncand] and f [batch][ncand*3] */
extern "C" int rkfd_cf_launch(rkfdCf *c, const double *dis, const int *active, const double *f, int flags, void *stream, char *err, int errlen);
/* flags of the last launch (0: none yet); host copies after waiting for it */
extern "C" int rkfd_cf_flags(const rkfdCf *c);
extern "C" int rkfd_cf_get(rkfdCf *c, double *point, double *wrench, int *count, double *genf, char *err, int errlen);
/* which: 0 point, 1 wrench, 2 count (an int array), 3 genf; NULL before the first launch that needed it */
extern "C" const void *rkfd_cf_dev(const rkfdCf *c, int which);

#endif /* RKFD_CF_HOST_H */
