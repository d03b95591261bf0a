/* rkfd_links_host.h - host side of the task-space read-out: the tables of rkfdLinksTab that the device model does not hold
 * (model link -> device link and its frame there, the chains' link lists, model-space masses and centres of mass), built from the
 * model and the merge the device-model builder kept (rkfdDevModelHost::part_off / part_idx / part_frame).  Shared by
 * rkfd_capi_links.hip and the lane emulator's harness. */
#ifndef RKFD_LINKS_HOST_H
#define RKFD_LINKS_HOST_H

#include <vector>
#include <string.h>
#include "rkfd_model.h"
#include "rkfd_devmodel_host.h"

struct rkfdLinksHostTab {
  std::vector<int> mdev, chain_off, chain_idx;
  std::vector<double> mframe, mvel, dorg, dpre, masscom;      /* masscom: mass [nlink_model] | com [nlink_model*3], the row layout of a per-instance table too */
};

static inline void rkfd_links_host_build(const rkfdModel *m, const rkfdDevModelHost *h, rkfdLinksHostTab *o)
{
  const int NLM = m->nlink, NL = h->dm.nlink, NCH = m->nchain;
  o->mdev.assign( NLM, 0 ); o->mframe.assign( (size_t)12*NLM, 0.0 );
  /* (the pseudo-links of a spherical joint have no parts: the model link belongs to the last of the three) */
  for( int r=0; r<NL; r++ )
    for( int q=h->part_off[r]; q<h->part_off[r+1]; q++ ) o->mdev[h->part_idx[q]] = r;
  memcpy( o->mframe.data(), h->part_frame, sizeof(double)*12*NLM );
  /* the velocity of a rigidly attached link in terms of its device link's, by the model's own recursion v_j = Ro_j' ( v_p + w_p x po_j ):
   * v_j = R_j' v + B_j w with B_j = Ro_j' ( B_p + C(po_j) R_p' ), C(x) w = w x x; a device link's own model link has B = 0 */
  o->mvel.assign( (size_t)9*NLM, 0.0 );
  for( int j=0; j<NLM; j++ ){
    const int pm = m->parent[j];
    if( m->jtype[j] != RKFD_JOINT_FIXED || pm < 0 ) continue;
    const double *og = &m->org[12*j], *Tp = &o->mframe[12*pm], *Bp = &o->mvel[9*pm];
    const double C[9] = { 0, og[11], -og[10], -og[11], 0, og[9], og[10], -og[9], 0 };
    double M[9];
    for( int a=0; a<3; a++ ) for( int b=0; b<3; b++ ) M[3*a+b] = Bp[3*a+b] + C[3*a]*Tp[3*b] + C[3*a+1]*Tp[3*b+1] + C[3*a+2]*Tp[3*b+2];
    for( int a=0; a<3; a++ ) for( int b=0; b<3; b++ ) o->mvel[9*j+3*a+b] = og[a]*M[b] + og[3+a]*M[3+b] + og[6+a]*M[6+b];
  }
  /* per device link: the org frame of its own model link and, in front of it, the model parent's frame and velocity block in the
   * device parent; the second and third device link of a spherical joint add nothing of either */
  o->dorg.assign( (size_t)12*NL, 0.0 ); o->dpre.assign( (size_t)21*NL, 0.0 );
  for( int r=0; r<NL; r++ ){
    const int jt = RKFD_LI_JT( h->dm.linfo[r] ), j = h->dm.orig[r], pm = m->parent[j];
    double *og = &o->dorg[12*r], *pre = &o->dpre[21*r];
    og[0] = og[4] = og[8] = 1.0; pre[0] = pre[4] = pre[8] = 1.0;
    if( jt == RKFD_DJT_SPHY || jt == RKFD_DJT_SPHZ ) continue;
    memcpy( og, &m->org[12*j], sizeof(double)*12 );
    if( pm >= 0 ){ memcpy( pre, &o->mframe[12*pm], sizeof(double)*12 ); memcpy( pre+12, &o->mvel[9*pm], sizeof(double)*9 ); }
  }
  o->chain_off.assign( NCH+1, 0 ); o->chain_idx.assign( NLM > 0 ? NLM : 1, 0 );
  for( int i=0; i<NLM; i++ ) if( m->chain[i] >= 0 && m->chain[i] < NCH ) o->chain_off[m->chain[i]+1]++;
  for( int c=0; c<NCH; c++ ) o->chain_off[c+1] += o->chain_off[c];
  {
    std::vector<int> cur( o->chain_off.begin(), o->chain_off.end()-1 );
    for( int i=0; i<NLM; i++ ) if( m->chain[i] >= 0 && m->chain[i] < NCH ) o->chain_idx[cur[m->chain[i]]++] = i;
  }
  o->masscom.resize( (size_t)4*NLM );
  memcpy( o->masscom.data(), m->mass, sizeof(double)*NLM );
  memcpy( o->masscom.data() + NLM, m->com, sizeof(double)*3*NLM );
}

/* ---- rkfd_capi_links.hip: the read-out of one batch (kernel, tables and result buffers on the batch's device), used by
 * rkfd_capi.hip's rkfdBatchUpdateLinks / GetLinks.  The caller has selected the device.  Failures return -1 with a message in err. */
struct rkfdLinks;
/* dm: the batch's device model with DEVICE pointers (linfo, anc, org are read through it) */
extern "C" rkfdLinks *rkfd_links_create(const rkfdModel *m, const rkfdDevModelHost *h, const rkfdDevModel *dm, int batch, char *err, int errlen);
extern "C" void rkfd_links_destroy(rkfdLinks *l);
/* one launch on `stream` from the device arrays dis / vel [batch][ndof].  par_mass / par_com: NULL, or the host copies
 * [batch][nlink_model] / [batch][nlink_model*3] of a table of per-instance parameters, uploaded again whenever par_gen differs
 * from the one of the last upload (only a read-out with RKFD_LINKS_COM looks at them) */
extern "C" int rkfd_links_launch(rkfdLinks *l, const double *dis, const double *vel, int flags, const double *par_mass, const double *par_com,
                                 int par_gen, void *stream, char *err, int errlen);
/* flags of the last launch (0: none yet); host copies after waiting for it (any pointer may be NULL) */
extern "C" int rkfd_links_flags(const rkfdLinks *l);
extern "C" int rkfd_links_get(rkfdLinks *l, double *R, double *p, double *v, double *com, double *comvel, char *err, int errlen);
/* which: 0 R, 1 p, 2 v, 3 com, 4 comvel; NULL before the first launch that needed it */
extern "C" const double *rkfd_links_dev(const rkfdLinks *l, int which);

#endif /* RKFD_LINKS_HOST_H */
