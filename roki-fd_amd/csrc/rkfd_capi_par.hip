/* rkfd_capi_par.hip - the step kernels of rkfd_capi.hip once more, built with RKFD_PARAMS = 1: every instance reads its link masses,
 * centres of mass, inertias, joint friction and contact-info constants at its own row of the table rkfdBatchSetParam made
 * (RKFD_PAR in device/rkfd_dev_base.h, par_stride in device/rkfd_dev_step.h).  A translation unit of its own, so that the kernels
 * of batches without a table stay what they are to the instruction; its resource report goes to kernel_resources_par.txt. */
#include <hip/hip_runtime.h>
#define RKFD_PARAMS 1
#define rkfd_kc rkfd_kc_par      /* (the constant table of rkfd_dev_base.h has a host-side symbol: one per translation unit) */
#include "rkfd_device.h"

#define RKFD_KERNEL_PAR(name, prof, vqp, pk, waves) \
extern "C" __global__ void __launch_bounds__(RKFD_WAVE, waves) \
name(rkfdDevModel m, rkfdDevState st, int first, int mode, int nsteps, int *errflag, const double *ctrl, int ctrl_stride, int par_stride) \
{ \
  extern __shared__ __attribute__((aligned(16))) char lds[]; \
  const int b = first + (int)blockIdx.x; \
  if( b >= st.batch ) return; \
  rkfd_instance<prof, vqp, pk>( m, st, b, lds, mode, nsteps, errflag, true, 0, prof ? nullptr : ctrl, ctrl_stride, par_stride ); \
}
/* (waves per SIMD as in rkfd_capi.hip) */
RKFD_KERNEL_PAR( rkfd_step_kernel_par, false, 0, false, 3 )
RKFD_KERNEL_PAR( rkfd_step_kernel_par_pk, false, 0, true, 3 )
RKFD_KERNEL_PAR( rkfd_step_kernel_par_vqp, false, 1, false, 2 )
RKFD_KERNEL_PAR( rkfd_step_kernel_par_vol, false, 2, false, 2 )
RKFD_KERNEL_PAR( rkfd_step_kernel_par_prof, true, 0, false, 3 )
RKFD_KERNEL_PAR( rkfd_step_kernel_par_prof_pk, true, 0, true, 3 )
RKFD_KERNEL_PAR( rkfd_step_kernel_par_prof_vqp, true, 1, false, 2 )
RKFD_KERNEL_PAR( rkfd_step_kernel_par_prof_vol, true, 2, false, 2 )

typedef void (*rkfdKernelPar)(rkfdDevModel, rkfdDevState, int, int, int, int *, const double *, int, int);
/* kind 0 plain, 1 packed contact matrix, 2 Vert QP, 3 Volume plugin; prof: the diagnostic instantiation */
extern "C" rkfdKernelPar rkfd_par_kernel(int kind, int prof)
{
  static const rkfdKernelPar k[2][4] = {
    { rkfd_step_kernel_par, rkfd_step_kernel_par_pk, rkfd_step_kernel_par_vqp, rkfd_step_kernel_par_vol },
    { rkfd_step_kernel_par_prof, rkfd_step_kernel_par_prof_pk, rkfd_step_kernel_par_prof_vqp, rkfd_step_kernel_par_prof_vol } };
  return k[prof ? 1 : 0][kind & 3];
}
