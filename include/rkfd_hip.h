/* rkfd_hip.h - C ABI of the MI355X (gfx950) batched rkFDUpdate path.
 *
 * Plain C: pointers, sizes and an opaque handle only (no torch / C++ types), so the
 * reference's C host code - or any FFI - can bind it.  Each entry point names the
 * reference interface it stands in for.  One process drives one GPU; a batch holds B
 * independent copies ("instances") of one world (all chains registered in one rkFD).
 *
 * Layout of every per-instance array handed across this boundary: instance-major,
 * x[b*stride + j] (b = instance).  Host pointers unless the name says "Dev".
 *
 * Every function returns 0 on success and a negative value on failure;
 * rkfdHipLastError() then describes the failure.  Without a usable GPU / kernel image
 * the calls FAIL (there is no CPU fallback).
 */
#ifndef RKFD_HIP_H
#define RKFD_HIP_H

#include "rkfd_model.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rkfdBatch rkfdBatch;

/* number of visible HIP devices (0 when none) */
int rkfdHipDeviceCount(void);
const char *rkfdHipLastError(void);

/* Creates device state for `batch` instances of world `m` on `device`.
 * Replaces, for the whole batch: rkFDCreate + rkFDChainReg* + rkFDUpdateInit's allocations
 * (reference src/rkfd_sim.c:32-54,188-235,552-558; rkFDCDUpdateInit src/rkfd_cd.c:22-31;
 * plugin _init src/rkfd_mlcp.c:312-325, src/rkfd_vert.c:350-368).  max_rigid = capacity of rigid
 * contact vertices solved per instance (MLCP plugin: 3*max_rigid <= 128; Vert plugin: pyramid*max_rigid
 * <= 192 - up to 8 vertices the QP keeps its factor in registers, up to 64 faces and unknowns one per lane, beyond that the
 * wide form with everything in LDS, one instance per CU; Volume plugin: rigid PAIRS in collision at once, at most 10 -
 * rigid pairs of convex polyhedra with at most 64 faces together are solved, the others are guarded:
 * status 4 when one comes into contact); exceeding it at run time is reported as an error by
 * rkfdBatchStatus. */
rkfdBatch *rkfdBatchCreate(const rkfdModel *m, int batch, int device, int max_rigid);
void rkfdBatchDestroy(rkfdBatch *b);

int rkfdBatchSize(const rkfdBatch *b);
int rkfdBatchDof(const rkfdBatch *b);

/* The Set / Get accessors below are SYNCHRONOUS and ordered after the batch's launches: each waits for the batch's internal
 * (split) streams and for the stream its LAST launch was given (rkfdBatchUpdateInit / Update / UpdateControlled[Dev] / Eval /
 * Restore / Reset[Dev] / UpdateLinks / UpdateJacobians / UpdateDynamics) before it copies - also when that stream was made with hipStreamNonBlocking, which the null stream of the
 * copies is not ordered against.  A value set is seen by every launch made after the call returns; a value read is what the
 * launches made before the call left.  Launches a caller spread over FURTHER streams of its own must be joined by the caller first
 * (rkfdBatchStatus on each, or its own events): only the stream of the last launch is known to the batch.  That stream must
 * still exist at the first accessor (or rkfdBatchStatus on it) after the launch: destroy it only after one of them has returned.
 * An error the launch left on the stream is the accessor's error.  rkfdBatchUpdateContactForces and rkfdBatchUpdateContactForcesDev
 * are launches in this sense too: the accessors wait for the stream they were given as for any of the above. */
/* rkFDChainSetDis / rkFDChainSetVel (reference src/rkfd_sim.c:277-287), all instances at once:
 * dis, vel are [batch][ndof] */
int rkfdBatchSetState(rkfdBatch *b, const double *dis, const double *vel);
/* fd->dis, fd->vel, fd->acc after rkFDUpdate (reference include/roki_fd/rkfd_sim.h:49-50); any may be NULL */
int rkfdBatchGetState(rkfdBatch *b, double *dis, double *vel, double *acc);
/* rkJointMotorSetInput on every link (reference example/chain/arm_box_test.c:21): [batch][nlink] */
int rkfdBatchSetMotorInput(rkfdBatch *b, const double *input);
/* contact-vertex state rkCDVert{type,_ref} and force f per candidate vertex
 * (consumed at reference src/rkfd_util.c:256-263, src/rkfd_mlcp.c:263-279): [batch][ncand], [batch][ncand*3] */
/* (entries of a candidate that is not in contact are reported as 0; the anchors `ref` are in the frame of the
 * other cell's link as registered - links rigidly attached to it are merged on the device, the boundary converts) */
int rkfdBatchGetContact(rkfdBatch *b, int *active, int *type, double *ref, double *f);
int rkfdBatchSetContact(rkfdBatch *b, const int *active, const int *type, const double *ref);
/* joint friction pivots rkJointFrictionPivot{type,prev_trq} (reference src/rkfd_util.c:289-311): [batch][nlink] */
int rkfdBatchGetPivot(rkfdBatch *b, int *type, double *prev_trq);
int rkfdBatchSetPivot(rkfdBatch *b, const int *type, const double *prev_trq);

/* breakable float joints (reference example/model/wall.ztk:51-53; RoKi rk_joint_brfloat, include/rkfd_model.h): 1 per link whose
 * joint has broken, 0 elsewhere, [batch][nlink].  State like the friction pivots: every launch reads it and writes it back. */
int rkfdBatchGetBroken(rkfdBatch *b, int *broken);
int rkfdBatchSetBroken(rkfdBatch *b, const int *broken);

/* rkFDUpdateInit's committing evaluation _rkFDUpdateRef (reference src/rkfd_sim.c:542-549,556).
 * stream: hipStream_t (NULL = default stream).  Asynchronous. */
int rkfdBatchUpdateInit(rkfdBatch *b, void *stream);
/* nsteps x rkFDUpdate (reference src/rkfd_sim.c:560-566) for every instance: one launch with the steps fused, or -
 * under split launches - nsteps rounds of one-step launches on the internal streams (same results).  Asynchronous. */
int rkfdBatchUpdate(rkfdBatch *b, int nsteps, void *stream);
/* nsteps x ( rkJointMotorSetInput on every link; rkFDUpdate ) - the reference drivers' control loop (example/chain/arm_box_test.c:
 * 16-21,69-82) - with the motor inputs of a control schedule u[batch][nsteps][nlink] (instance-major: u[(b*nsteps + k)*nlink + l] is
 * the input of link l in step k of instance b).  Bit-identical to nsteps x ( rkfdBatchSetMotorInput( u[:, k, :] );
 * rkfdBatchUpdate( 1 ) ), in the launches rkfdBatchUpdate makes; afterwards the batch's motor input is the last row u[:, nsteps-1, :].
 * Host schedule: copied into a buffer of the batch before the call returns (u may be reused at once), then to the device in stream
 * order.  Asynchronous. */
int rkfdBatchUpdateControlled(rkfdBatch *b, int nsteps, const double *u, void *stream);
/* the same with the schedule on the batch's device, read in stream order after `stream` (no copy: schedules sampled on the GPU);
 * the caller keeps u_dev unchanged until the steps are done (rkfdBatchJoin on a stream it then orders by, or rkfdBatchStatus) */
int rkfdBatchUpdateControlledDev(rkfdBatch *b, int nsteps, const double *u_dev, void *stream);
/* one evaluation _rkFDUpdate (doUpRef=0) or _rkFDUpdateRef (doUpRef=1) at the current state
 * (reference src/rkfd_sim.c:533-549): fills acc and the contact forces.  Asynchronous. */
int rkfdBatchEval(rkfdBatch *b, int doUpRef, void *stream);
/* Split launches: the batch goes out as `nsplit` (1..8) kernels over contiguous parts on internal streams.  The
 * instances are independent, so the parts need not wait for each other: the thinly occupied tail of one
 * step of one part then overlaps the next step of another (+20 % at 4096 instances per GPU).  The parts start
 * after whatever `stream` holds at the time of the call; `stream` itself does NOT wait for them until
 * rkfdBatchJoin( b, stream ) or rkfdBatchStatus( b, stream ); the host-side accessors (Get / Set) wait for the internal
 * streams and for `stream` of the last launch, at every nsplit.
 * nsplit = 1 (default): one launch on the caller's stream, plain stream order. */
int rkfdBatchSetSplit(rkfdBatch *b, int nsplit);
/* Under split launches a call of n steps goes out as rounds of launches of at most `steps` steps each (default 5; worlds under
 * the Vert plugin keep one fused launch per part): one step per launch reloads the instance's state and the world's tables every
 * step, all n in one launch hold the slots while the rest of the batch waits - measured on config 4, rollouts of 25 steps, 1 / 2 /
 * 3 / 5 / 9 / 13 / 25 steps per launch: 11.51 / 11.63 / 11.65 / 11.82 / 11.79 / 11.82 / 11.76 M steps/s.  Results do not depend
 * on it (tests/test_gpu_edge.py: fused vs single-step launches bit for bit). */
int rkfdBatchSetStepsPerLaunch(rkfdBatch *b, int steps);
/* Compile the step kernel for THIS world (hipRTC, a few seconds): the same device code with the world's dimensions
 * as literals, so that the LDS layout, loop bounds and table strides fold into immediates (+7 % steps/s on the
 * 30-DoF humanoid).  Results are bit-identical to the generic kernels, which stay in use for the profiling entry
 * point.  Self-contained: the library carries the device sources it hands to hipRTC, and binds hipRTC and the compiler
 * library beside it (the ROCm it was built with; RKFD_ROCM_LIBDIR overrides) in a private link namespace, so neither files
 * beside the library nor the order in which the host program loaded other ROCm-bundling libraries matter; 0, or -1 with
 * a message (the generic kernels remain in use then).  rkfdSpecializeCompile: the compile step alone, without a GPU - bytes
 * of code object, or -1. */
int rkfdBatchSpecialize(rkfdBatch *b);
int rkfdSpecializeCompile(const rkfdModel *m, int max_rigid);
int rkfdSpecializeCompileW(const rkfdModel *m, int max_rigid, int ipw);      /* ipw: instances per wavefront, 1 or 2 (below) */
/* par = 1: the kernel for batches that carry a table of per-instance parameters (rkfdBatchSetParam below); `make spec` makes both */
int rkfdSpecializeCompileP(const rkfdModel *m, int max_rigid, int ipw, int par);
/* Ahead-of-time kernels: a specialised kernel is a function of the world's dimensions and the device sources only, so its code
 * object is kept in a directory beside the library (`spec/`; RKFD_SPEC_DIR overrides, RKFD_SPEC_STORE=0 switches the store off),
 * keyed by a hash of everything that goes into it.  `make spec` fills it for the worlds of BASELINE.json's configurations at
 * build time, so that those need no run-time compiler at all; other worlds are compiled on first use and kept.  1 when the
 * last rkfdBatchSpecialize / rkfdSpecializeCompile was served from the store, else 0 (measurement / test aid). */
int rkfdSpecializeLastFromStore(void);
/* test aid: XOR mask over the kernel variants of the batches created AFTER the call (4: the Vert QP's Q = A'A off the matrix
 * cores, 8: grouped Gauss-Seidel off, 32: its sweep-order storage off); returns the previous mask.  0 = the product's defaults. */
int rkfdDebugVariants(int mask);
/* Instances per wavefront of the world-specific kernel: 1 (default: one instance has the 64 lanes) or 2 (two instances share a
 * wavefront, 32 lanes each: half the instruction issue per instance where an instance leaves most of the 64 lanes idle).  Call
 * before rkfdBatchSpecialize; needs a world of at most 32 device links, 32 joint coordinates, 32 contact slots and 16 rigid
 * contact vertices under the MLCP plugin or with elastic contacts only (else -1 with a message, one per wavefront stays).
 * Results are bit-identical to one instance per wavefront.  rkfdBatchInstancesPerWave: what the launches really use. */
int rkfdBatchSetInstancesPerWave(rkfdBatch *b, int ipw);
int rkfdBatchInstancesPerWave(const rkfdBatch *b);
/* MEASURE which of the two is faster for this world, on this device, at this batch size, and keep it: nsteps steps under
 * either from the batch's present state (set one and call rkfdBatchUpdateInit first), which is put back afterwards; an
 * earlier rkfdBatchSnapshot stays as it was.  Returns the chosen count, -1 on error; ms[2] (may be NULL): the milliseconds
 * measured for 1 and 2 (ms[1] < 0: the world is not eligible for two).  Safe by construction: both give the same bits. */
int rkfdBatchTuneInstancesPerWave(rkfdBatch *b, int nsteps, double *ms);
int rkfdBatchJoin(rkfdBatch *b, void *stream);
/* measurement aid: with on = 1 every launch is bracketed by HIP events on the stream it runs on;
 * rkfdBatchLaunchTiming synchronises the device and returns their number and summed duration */
int rkfdBatchTimeLaunches(rkfdBatch *b, int on);
int rkfdBatchLaunchTiming(rkfdBatch *b, int *launches, double *total_ms);

/* waits for the stream-ordered work, then reports device-side conditions:
 * 0 ok, 1 rigid contact met without a rigid solver set up (max_rigid = 0),
 * 2 contact capacity exceeded - more rigid contact vertices (Volume plugin: pairs in collision, or contact-plane
 * conditions of a pair: 8) than max_rigid, or more rigid + elastic contact
 * vertices than the active-contact slots (max_rigid when the world has no elastic pairs, else max(max_rigid, 16)
 * capped by the candidate count); the vertices beyond the capacity were dropped -, 3 the Vert plugin's QP ran
 * out of iterations (256) or of basis history (64), 4 Volume plugin: a GUARDED pair came into contact - a rigid pair with a
 * shape that is not convex, or with more than 64 faces together, cannot be clipped on the device; such a world is accepted
 * (the reference's humanoid mighty.ztk, whose body meshes are not convex, stands and walks on its convex soles) and the
 * plugin's own collision test watches those pairs -, 5 rkfdBatchReset / ResetDev: a slot value that names no row (that instance
 * was left as it was); negative: HIP error.  rkfdHipLastError() describes a
 * non-zero status.  A condition is reported ONCE: the call clears the device-side flag, so the next status tells
 * what happened after this one (when several conditions occurred since the last call, the last one written wins). */
int rkfdBatchStatus(rkfdBatch *b, void *stream);

/* Mean number of rigid / elastic contact vertices per instance at the committing evaluation of the rkFDUpdate
 * steps run since the last reset (the length of the plugin's vertex lists, reference src/rkfd_mlcp.c:327-345,
 * src/rkfd_vert.c:380-392), and the number of instance-steps counted.  Measurement aid: tells what contact
 * problem a timed region really solved.  Synchronises the device.  Any output may be NULL. */
int rkfdBatchContactStats(rkfdBatch *b, int reset, double *mean_rigid, double *mean_elastic, long long *instance_steps);

/* MPC-style rollouts: rkfdBatchSnapshot keeps a device-resident copy of the whole per-instance state (joint
 * state, accelerations, friction pivots, contact-vertex state and forces; synchronous), rkfdBatchRestore puts it
 * back in stream order (one small copy kernel per part, no host traffic) - the start of the next rollout from the
 * same states.  The reference has no counterpart: a caller would re-run rkFDChainSetDis / SetVel per instance
 * (reference src/rkfd_sim.c:277-287) and rkFDUpdateInit. */
int rkfdBatchSnapshot(rkfdBatch *b);
int rkfdBatchRestore(rkfdBatch *b, void *stream);

/* ---- per-instance reset on the device from a bank of start states ------------------------------------------------------
 * rkfdBatchRestore puts EVERY instance back; an RL or sampling loop whose episodes end at different times starts ONE instance over
 * while its neighbours run on.  The bank is `nslots` rows on the batch's device, each the complete state of one instance - what
 * Snapshot / Restore keep: dis, vel, acc, friction pivots, broken flags, contact-vertex state, anchors and forces; motor input,
 * parameters and the contact statistics are not state here either.  It is separate from the whole-batch snapshot, and a batch that
 * never reserves one allocates nothing.  The rows come from LIVE instances: set K start states in K instances, rkfdBatchUpdateInit,
 * optionally some steps, rkfdBatchBankStore - the rows then hold consistent accelerations, pivots, anchors and forces, and an
 * instance reset from a row continues bit for bit as the stored instance did (under the same motor input and parameters).  One
 * launch of rkfd_reset_kernel (a kernel of its own: the step kernels are untouched), one wavefront per instance; an instance that
 * keeps its state costs one load and one branch.  The reference has no counterpart: its caller re-runs rkFDChainSetDis / SetVel
 * (reference src/rkfd_sim.c:277-287) and rkFDUpdateInit on one rkFD; a masked rkfdBatchUpdateInit is not given (DEVIATIONS.md). */
int rkfdBatchBankReserve(rkfdBatch *b, int nslots);   /* (re)allocates, contents undefined; 0 frees; synchronous */
int rkfdBatchBankSize(const rkfdBatch *b);            /* 0 when none; -1 null batch */
/* rows slot .. slot+count-1  <-  live state of instances first .. first+count-1.
 * Synchronous and ordered after the batch's launches like rkfdBatchSnapshot. */
int rkfdBatchBankStore(rkfdBatch *b, int slot, int first, int count);
enum { RKFD_RESET_KEEP = -1, RKFD_RESET_SNAPSHOT = -2 };
/* slots[batch], int32: s in [0, nslots)       -> instance i gets bank row s
 *                     RKFD_RESET_KEEP         -> instance i is not touched
 *                     RKFD_RESET_SNAPSHOT     -> instance i gets ITS OWN row of rkfdBatchSnapshot (a masked Restore)
 * anything else (including SNAPSHOT when no snapshot was taken, and any s >= 0 when there is no bank): the instance is not
 * touched and rkfdBatchStatus reports the status 5, once, like the other conditions.
 * Asynchronous, in stream order; under split launches every part resets itself on its own internal stream, in order with its
 * steps, as rkfdBatchRestore does. */
int rkfdBatchReset(rkfdBatch *b, const int *slots, void *stream);        /* host array: staged in a pinned buffer of the batch before
                                                                           the call returns, reusable at once (as the control schedule is) */
int rkfdBatchResetDev(rkfdBatch *b, const int *slots_dev, void *stream); /* on the batch's device, read in stream order; the caller
                                                                           keeps it unchanged until the reset is done */

/* ---- per-instance physical parameters (domain randomisation) --------------------------------------------------------
 * A batch is `batch` copies of one world; these calls let every instance have its OWN link masses, centres of mass, inertias, joint
 * friction and contact-info constants - what a caller of the reference gets by building one rkFD per world from its own chain
 * and contact-info files.  Parameters are addressed in MODEL space (the links and contact infos of the rkfdModel the batch was made
 * from, not the device's merged links), one key at a time, values[batch][width] instance-major.  Instance i of a batch that
 * carries parameters P_i gives, bit for bit, what a plain batch gives on a copy of the model that holds P_i.
 *   rkfdBatchSetParam: synchronous like rkfdBatchSetState - waits for the batch's launches (its internal streams and the stream of
 *     its last launch; launches the caller spread over other streams of its own must be joined first), takes effect from the next
 *     launch.  The first Set on a batch that runs a world-specific kernel (rkfdBatchSpecialize) also fetches the kernel built for
 *     batches with a table: from the store `make spec` fills, else a run-time compile of a few seconds, once per world; a Set that
 *     fails for any reason (-1) has changed nothing - neither the table nor the kernel in use.  It
 *     touches no state: friction pivots, contact anchors and broken flags stay as they are.  values = NULL: this key back to the
 *     model's value in every instance.  Refused with -1 and a message (rkfdHipLastError), the table left as it was: an unknown key, a
 *     value that is not finite, a negative mass, a mass of 0 for a link whose mass is positive in the model.
 *   rkfdBatchGetParam: what the next launch will use (the model's values if the key was never set).
 *   rkfdBatchClearParams: every key back to the model; frees the table.  rkfdBatchHasParams: 1 while the batch carries a table.
 * rkfdBatchSnapshot / rkfdBatchRestore neither save nor restore parameters: they are not state.  Every launch honours the table:
 * rkfdBatchUpdateInit / Update / UpdateControlled(Dev) / Eval / Profile, whatever rkfdBatchSpecialize, SetSplit, SetStepsPerLaunch,
 * SetInstancesPerWave or TuneInstancesPerWave chose (the tuning measures with the table in place and keeps it).
 * Topology, geometry, joint types, motor constants, dt and the solver's settings stay per world (DEVIATIONS.md).
 * Cost: 17 device links + 6 contact infos doubles per instance on the device (config 4: about 4 KB), the same again in model
 * space on the host, allocated at the first Set. */
enum { RKFD_PAR_MASS, RKFD_PAR_COM, RKFD_PAR_INERTIA,                            /* per link: 1, 3, 9 doubles */
       RKFD_PAR_STIFF, RKFD_PAR_VISC, RKFD_PAR_COULOMB, RKFD_PAR_SFRIC,          /* per link: 1 each */
       RKFD_PAR_CI_SF, RKFD_PAR_CI_KF, RKFD_PAR_CI_K, RKFD_PAR_CI_L, RKFD_PAR_CI_E, RKFD_PAR_CI_V,   /* per contact info */
       RKFD_PAR_COUNT };
int rkfdBatchParamWidth(const rkfdBatch *b, int which);                 /* doubles per instance: nlink*{1,3,9} or nci; -1: bad key */
int rkfdBatchSetParam(rkfdBatch *b, int which, const double *values);   /* [batch][width]; NULL: this key back to the model's value */
int rkfdBatchGetParam(rkfdBatch *b, int which, double *values);         /* what the next launch will use */
int rkfdBatchClearParams(rkfdBatch *b);                                  /* all keys back to the model; frees the table */
int rkfdBatchHasParams(const rkfdBatch *b);

/* diagnostic launch: nsteps x rkFDUpdate with in-kernel phase stamps.  out is [batch][32]
  * (RKFD_NPROF = 32 per instance) shader-clock cycles: kinematics, collision+penalty, sweep 2, sweep 3 (both
 * passes), MLCP, tail, MLCP matrix, whole launch, then finer stamps inside sweep 2 (8-13), MLCP (14, 15, 21-23),
 * kinematics (16-20) and the Vert QP (24-30); tools/prof_phases.py names them.
 * Synchronous; not for timing runs (the stamps serialise the phases). */
int rkfdBatchProfile(rkfdBatch *b, int nsteps, unsigned long long *out);

/* device pointers to the live state ([batch][ndof] doubles), for zero-copy consumers
 * (e.g. an RCCL all-gather of final states) */
double *rkfdBatchDevDis(rkfdBatch *b);
double *rkfdBatchDevVel(rkfdBatch *b);
double *rkfdBatchDevAcc(rkfdBatch *b);

/* kernel resource facts for measurement: LDS bytes per instance */
int rkfdBatchLdsBytes(const rkfdBatch *b);
/* instances that can be resident on one compute unit at a time: the HIP runtime's occupancy answer for the step
 * kernel (registers, LDS), corrected for the 1280-byte pieces in which the hardware allocates LDS; -1 on error */
int rkfdBatchResidency(const rkfdBatch *b);
/* the same figure computed on the host for a model and contact capacity (no GPU needed) */
int rkfdLdsBytesFor(const rkfdModel *m, int max_rigid);

/* ---- task-space read-out: link poses, link velocities and chain centres of mass, computed ON THE DEVICE from the live state ----
 * What an MPC / RL cost is made of (base height and tilt, foot and hand positions, the centre of mass, a link's velocity) without
 * copying the joint state to the host and re-doing the forward kinematics there.  One kernel launch (rkfd_links_kernel, a kernel
 * of its own: the step kernels are untouched) computes, for every instance,
 *   R      [batch][nlink][3][3]  orientation of every MODEL link, row-major, link -> world
 *   p      [batch][nlink][3]     position of its origin, world (absolute)
 *   v      [batch][nlink][6]     (linear, angular) velocity of the link origin, in the link's OWN frame (DEVIATIONS.md item 1)
 *   com    [batch][nchain][3]    centre of mass of every chain, world:  sum m_i ( p_i + R_i c_i ) / sum m_i
 *   comvel [batch][nchain][3]    its velocity, world:                   sum m_i R_i ( v_i + w_i x c_i ) / sum m_i
 * (a chain without mass reports zeros; a batch with a table of per-instance parameters uses the instance's masses and centres of
 * mass).  Links are the model's links, as everywhere at this boundary: rigidly attached links the device merges and the three
 * device links of a spherical joint are resolved here.  A breakable float joint sits where its six coordinates put it, broken
 * or not.  Link accelerations, contact point positions, a subset of links and per-step values inside a fused launch are not given
 * (DEVIATIONS.md): read per step, or at the end of a rollout.
 * A batch that never calls these allocates nothing and launches nothing; snapshot / restore do not save the results (derived data). */
enum { RKFD_LINKS_POSE = 1, RKFD_LINKS_VEL = 2, RKFD_LINKS_COM = 4 };
int rkfdBatchLinkNum(const rkfdBatch *b);            /* model links */
int rkfdBatchChainNum(const rkfdBatch *b);
/* computes the selected quantities from the live state, in stream order after everything the batch has launched (joins the
 * internal split streams onto `stream` first, as rkfdBatchJoin does); asynchronous; changes no state */
int rkfdBatchUpdateLinks(rkfdBatch *b, int flags, void *stream);
/* host copies of the last rkfdBatchUpdateLinks (waits for it); any pointer may be NULL; -1 with a message when a requested
 * quantity was not part of the last read-out or none was made */
int rkfdBatchGetLinks(rkfdBatch *b, double *R, double *p, double *v, double *com, double *comvel);
/* device pointers to the same buffers (owned by the batch, allocated at the first read-out that needs them, stable afterwards;
 * NULL before) */
const double *rkfdBatchDevLinkAtt(rkfdBatch *b);
const double *rkfdBatchDevLinkPos(rkfdBatch *b);
const double *rkfdBatchDevLinkVel(rkfdBatch *b);
const double *rkfdBatchDevCom(rkfdBatch *b);
const double *rkfdBatchDevComVel(rkfdBatch *b);

/* ---- task-space Jacobians: the map from the joint rates to the velocities the read-out reports, computed ON THE DEVICE ----
 * What lies between a task-space cost and a joint command (operational-space control, whole-body QPs, a balance controller on the
 * centre of mass, J' f for a desired contact force, the gradient of a task-space cost).  A SITE is a model link plus a point in
 * that link's frame.  One kernel launch (rkfd_jac_kernel, a kernel of its own: the step kernels and the read-out are untouched)
 * computes, for every instance,
 *   J    [batch][nsite][6][ndof]   world frame: rows 0-2 times vel = velocity of the site point, rows 3-5 times vel = angular
 *                                  velocity of the site's link - with R, ( v, w ) of the read-out at the same state:
 *                                  J[s][0:3] vel = R ( v + w x point ),  J[s][3:6] vel = R w
 *   Jcom [batch][nchain][3][ndof]  world frame: Jcom[c] vel = comvel[c] of the read-out (the instance's own masses and centres of
 *                                  mass when the batch carries a table of per-instance parameters; zeros for a chain without mass)
 * `vel` is the packed rate vector of rkfdBatchSetState / GetState, so the columns are derivatives with respect to the RATES
 * (DEVIATIONS.md items 1-2): the scalar rate of a revolute / prismatic joint about / along local z, ( v, w ) of a float or breakable
 * float joint and w of a spherical joint in the joint-origin frame - not derivatives with respect to the angle-axis coordinates.
 * A breakable float joint contributes its six columns whether it has broken or not, as in the read-out.  Columns of coordinates that
 * do not move the site (other chains, joints that are no ancestors of its link) are exactly 0.0.  J is the exact linear map of the
 * model's own velocity recursion (readout/rkfd_jac.h), not axis x lever arm on composed world frames.
 * A batch that never calls these allocates nothing and launches nothing; snapshot / restore / reset do not touch the results
 * (derived data). */
enum { RKFD_JAC_SITES = 1, RKFD_JAC_COM = 2 };
/* the sites of the following launches: link[nsite] model links, point[nsite][3] in the link's frame or NULL for the link origins.
 * Synchronous (waits for a Jacobian launch in flight); nsite = 0 clears the sites; the result buffer is reallocated only when
 * nsite changes.  -1 with a message, the previous sites staying in place, for a link outside [0, nlink), a point that is not finite
 * or nsite > 64 */
int rkfdBatchSetJacobianSites(rkfdBatch *b, int nsite, const int *link, const double *point);
int rkfdBatchJacobianSiteNum(const rkfdBatch *b);
/* computes the selected Jacobians from the live state, in stream order after everything the batch has launched (joins the internal
 * split streams onto `stream` first, as rkfdBatchUpdateLinks does); asynchronous; changes no state.  -1 with a message for
 * RKFD_JAC_SITES without sites, flags 0 or unknown bits */
int rkfdBatchUpdateJacobians(rkfdBatch *b, int flags, void *stream);
/* host copies of the last rkfdBatchUpdateJacobians (waits for it); either pointer may be NULL; -1 with a message when a requested
 * one was not part of the last launch, none was made, or the sites were replaced since */
int rkfdBatchGetJacobians(rkfdBatch *b, double *J, double *Jcom);
/* device pointers to the same buffers (owned by the batch, allocated at the first launch that needs them, stable while nsite stays;
 * NULL before, and for J after nsite changed until the next launch) */
const double *rkfdBatchDevJacobian(rkfdBatch *b);
const double *rkfdBatchDevComJacobian(rkfdBatch *b);

/* ---- joint-space dynamics: the other half of the equation of motion, computed ON THE DEVICE ----------------------------------
 *   M(q) qdd + h(q, qd) = tau + J_c' f
 * What an operational-space controller ( ( J M^-1 J' )^-1 ), a whole-body QP (M and h in its equality constraint), gravity
 * compensation ( g(q) ) and an inverse-dynamics feed-forward ( M qdd_des + h ) need beside the Jacobians.  One kernel launch
 * (rkfd_dyn_kernel, a kernel of its own: the step kernels, the read-out and the Jacobians are untouched) computes, for every
 * instance from its live dis / vel,
 *   M [batch][ndof][ndof]  the joint-space inertia matrix with respect to the packed RATES - the `vel` vector of rkfdBatchSetState,
 *                          the coordinates of the columns of J (DEVIATIONS.md items 1-2), not derivatives of the angle-axis
 *                          coordinates -: 0.5 vel' M vel is the kinetic energy of the velocities the read-out reports.  Exactly
 *                          symmetric (M[i][j] and M[j][i] are the same bits); blocks between coordinates of different chains, and
 *                          between coordinates where neither owner is an ancestor of the other, are exactly 0.0
 *   h [batch][ndof]        the bias force rnea( q, qd, 0 ): Coriolis and centrifugal terms plus gravity (RKFD_G along -z, as in the
 *                          step); the sign is such that M qdd + h is the generalised force on the coordinates
 *   g [batch][ndof]        gravity alone, rnea( q, 0, 0 )
 * Generalised forces: a revolute / prismatic joint takes the scalar about / along local z, a float or breakable float joint (force,
 * moment about the link origin) on the joint-origin axes, a spherical joint the moment on those axes.  A breakable float joint is a
 * float joint here whether it has broken or not, as in the read-out and the Jacobians: a caller who wants the intact system drops its
 * six rows and columns (DEVIATIONS.md).  NOT part of h: joint friction (it depends on the pivot state), actuator torques, and contact
 * forces - the caller has J and rkfdBatchGetContact for those.  A batch with a table of per-instance parameters uses the instance's
 * own masses, centres of mass and inertias.
 * RKFD_DYN_ROTOR (with RKFD_DYN_MASS) adds mot_gear^2 x mot_inertia of the DC-motor joints to the diagonal, the reflected rotor and
 * gear inertia of DEVIATIONS.md item 5: with it M acc + h closes against the step's own accelerations with the motor's torque less
 * that term; without it M is the rigid-body matrix.
 * Worlds of more than 64 joint coordinates are refused at the first call with a message, as the Jacobians refuse them; so is a world
 * whose tables for one instance exceed the LDS of a workgroup (the message names the bytes).
 * A batch that never calls these allocates nothing and launches nothing; snapshot / restore / reset do not touch the results
 * (derived data). */
enum { RKFD_DYN_MASS = 1, RKFD_DYN_BIAS = 2, RKFD_DYN_GRAVITY = 4, RKFD_DYN_ROTOR = 8 };
/* computes the selected quantities from the live state, in stream order after everything the batch has launched (joins the internal
 * split streams onto `stream` first, as rkfdBatchUpdateLinks does); asynchronous; changes no state.  -1 with a message for flags 0,
 * unknown bits, or RKFD_DYN_ROTOR without RKFD_DYN_MASS */
int rkfdBatchUpdateDynamics(rkfdBatch *b, int flags, void *stream);
/* host copies of the last rkfdBatchUpdateDynamics (waits for it); any pointer may be NULL; -1 with a message when a requested
 * quantity was not part of the last launch or none was made */
int rkfdBatchGetDynamics(rkfdBatch *b, double *M, double *h, double *g);
/* device pointers to the same buffers (owned by the batch, allocated at the first launch that needs them, stable afterwards; NULL
 * before) */
const double *rkfdBatchDevMassMatrix(rkfdBatch *b);
const double *rkfdBatchDevBias(rkfdBatch *b);
const double *rkfdBatchDevGravity(rkfdBatch *b);

/* ---- contact read-out: the contact term J_c' f of the equation of motion, computed ON THE DEVICE --------------------------------
 * The step kernels keep the force of every candidate contact vertex (rkfdBatchGetContact: a synchronous host copy, indexed by
 * candidate).  One kernel launch (rkfd_cf_kernel, a kernel of its own: the step kernels, the read-out, the Jacobians and the dynamics
 * are untouched) turns them, for every instance from its live dis, into what an observation, a termination test or a whole-body
 * controller needs, in MODEL space - model links as rkfdModel numbers them, the packed joint rates of the columns of J and M:
 *   point  [batch][ncand][3]   the world position x_j = p_own + R_own v_j of every candidate vertex, active or not
 *   wrench [batch][nlink][6]   the net contact wrench on every model link in world axes: rows 0-2 the force, rows 3-5 the moment about
 *                              the link's own origin (the p of rkfdBatchUpdateLinks).  An active candidate j gives +f_j at x_j to the
 *                              link that owns the vertex (cand_side) and -f_j at x_j to the other link of its pair; links of chains
 *                              without coordinates (a floor) get theirs too
 *   count  [batch][nlink]      (int) the active candidates that touch the link, on either side
 *   genf   [batch][ndof]       sum_j J_j' f_j = sum_l J_l[0:3]' F_l + J_l[3:6]' N_l with J_l what rkfdBatchUpdateJacobians gives for the
 *                              site ( link l, its origin ) and ( F_l, N_l ) the row of wrench: M qdd + h = tau + genf.  Exactly 0.0 on
 *                              coordinates whose link is no ancestor of a touched link; a breakable float joint gets its six entries
 *                              whether it has broken or not, as in J
 * A candidate whose flag is 0 contributes nothing, whatever its force entry holds (the step leaves stale values there).  No mass and
 * no other per-instance parameter enters.  Worlds under the Volume plugin are refused at the first call with a message (that plugin
 * produces no per-vertex forces), as are worlds of more than 64 joint coordinates and worlds whose tables for one instance exceed the
 * LDS of a workgroup (the message names the bytes).  A batch that never calls these allocates nothing and launches nothing; snapshot /
 * restore / reset do not touch the results (derived data). */
enum { RKFD_CF_POINT = 1, RKFD_CF_WRENCH = 2, RKFD_CF_GENF = 4 };
/* computes the selected quantities (RKFD_CF_WRENCH: wrench and count) from the live dis and the batch's own candidate flags and forces,
 * in stream order after everything the batch has launched (joins the internal split streams onto `stream` first, as
 * rkfdBatchUpdateLinks does); asynchronous; changes no state.  -1 with a message for flags 0 or unknown bits */
int rkfdBatchUpdateContactForces(rkfdBatch *b, int flags, void *stream);
/* the same launch with the flags and forces of the caller - hypothesised forces of a contact-implicit controller, or of a solver of
 * its own -: active_dev [batch][ncand] (int), f_dev [batch][ncand*3] on the batch's device, read in stream order after `stream` (no
 * copy); they must stay unchanged until the launch is done (rkfdBatchStatus on that stream, or any accessor) */
int rkfdBatchUpdateContactForcesDev(rkfdBatch *b, int flags, const int *active_dev, const double *f_dev, void *stream);
/* host copies of the last launch (waits for it); any pointer may be NULL; -1 with a message when a requested quantity was not part of
 * the last launch or none was made */
int rkfdBatchGetContactForces(rkfdBatch *b, double *point, double *wrench, int *count, double *genf);
/* device pointers to the same buffers (owned by the batch, allocated at the first launch that needs them, stable afterwards; NULL
 * before) */
const double *rkfdBatchDevContactPoint(rkfdBatch *b);
const double *rkfdBatchDevContactWrench(rkfdBatch *b);
const int *rkfdBatchDevContactCount(rkfdBatch *b);
const double *rkfdBatchDevContactGenForce(rkfdBatch *b);

/* ---- the node level: all the GPUs of one node from ONE process, host code in C -------------------------------------
 * SURVEY 8e / north star: "independent MPC-style rollouts shard embarrassingly across the 8 GPUs of one node with an
 * RCCL-over-xGMI gather of final states only".  The instances of a batch are independent (one rkFD never references another),
 * so device k simulates the contiguous block [lo, hi) of the `total` instances (remainders to the low devices), model constants
 * replicated, NO per-step communication; every device has its own host thread and HIP stream inside the library, and the only
 * collective is one ncclAllGather of the final {dis, vel} per rollout (librccl is bound at run time; RKFD_RCCL_LIB names
 * another file).  The reference is single-threaded C on one core and has no counterpart; a caller of the reference would run
 * one rkFD per instance (reference example/chain/boxdrop_test.c:22-54).
 * ndev <= 0: all visible devices; devices: their HIP ordinals, or NULL for 0 .. ndev-1.  Calls return 0 / negative like the
 * rkfdBatch calls (rkfdHipLastError names the device); rkfdNodeStatus returns the largest rkfdBatchStatus of the devices. */
typedef struct rkfdNode rkfdNode;
rkfdNode *rkfdNodeCreate(const rkfdModel *m, int total, int max_rigid, int ndev, const int *devices);
void rkfdNodeDestroy(rkfdNode *n);
int rkfdNodeDevices(const rkfdNode *n);
int rkfdNodeSize(const rkfdNode *n);
/* shard k: its HIP device and its block of instances [lo, hi); the rkfdBatch behind it (for the per-batch accessors) */
int rkfdNodeShard(const rkfdNode *n, int k, int *device, int *lo, int *hi);
rkfdBatch *rkfdNodeBatch(rkfdNode *n, int k);
/* host arrays over ALL instances, [total][ndof] / [total][nlink]: scattered to / collected from the devices' shards; ordered after
 * the node's launches like the rkfdBatch accessors (each shard waits for its device's stream), as are the per-batch accessors on
 * rkfdNodeBatch( n, k ) */
int rkfdNodeSetState(rkfdNode *n, const double *dis, const double *vel);
int rkfdNodeSetMotorInput(rkfdNode *n, const double *input);
int rkfdNodeGetState(rkfdNode *n, double *dis, double *vel, double *acc);      /* plain copies, no collective; any may be NULL */
/* rkfdBatchSpecialize / SetSplit / UpdateInit / Update / Snapshot / Restore / Status on every device, each issued by the
 * device's own host thread on the device's own stream; the call returns when every thread has issued its launches (the GPUs run
 * on; Status and Gather wait for them) */
int rkfdNodeSpecialize(rkfdNode *n);
int rkfdNodeSetSplit(rkfdNode *n, int nsplit);
int rkfdNodeSetStepsPerLaunch(rkfdNode *n, int steps);        /* rkfdBatchSetStepsPerLaunch on every device */
int rkfdNodeTuneInstancesPerWave(rkfdNode *n, int nsteps);    /* rkfdBatchTuneInstancesPerWave on every device (each keeps what is faster there) */
int rkfdNodeUpdateInit(rkfdNode *n);
int rkfdNodeUpdate(rkfdNode *n, int nsteps);
int rkfdNodeSnapshot(rkfdNode *n);
int rkfdNodeRestore(rkfdNode *n);
int rkfdNodeStatus(rkfdNode *n);
/* rkfdBatchUpdateControlled on every device: u is the host schedule of ALL instances, [total][nsteps][nlink]; each device's thread
 * copies its shard's contiguous block on the device's own stream, in order with its steps */
int rkfdNodeUpdateControlled(rkfdNode *n, int nsteps, const double *u);
/* rkfdBatchSetParam / rkfdBatchClearParams on every device: values is the host array of ALL instances, [total][width], sharded like
 * rkfdNodeSetState (NULL: the key back to the model's value everywhere).  Nothing is changed on any device when one refuses. */
int rkfdNodeSetParam(rkfdNode *n, int which, const double *values);
int rkfdNodeClearParams(rkfdNode *n);
/* the bank of start states on every device (replicated, like the model): rkfdNodeBankStore takes GLOBAL instance indices, reads the
 * rows from the shards that own them and writes them to every device's bank (through the host).  rkfdNodeReset: slots[total] on the
 * host, sharded like rkfdNodeSetState, issued on each device's own thread and stream; nothing is changed on any device when one
 * refuses. */
int rkfdNodeBankReserve(rkfdNode *n, int nslots);
int rkfdNodeBankStore(rkfdNode *n, int slot, int first, int count);
int rkfdNodeReset(rkfdNode *n, const int *slots);
/* rkfdBatchUpdateLinks( flags ) on every device's own thread and stream, then host arrays over ALL instances in instance order
 * (shapes as rkfdBatchGetLinks with batch = total; pointers of quantities `flags` does not select must be NULL) */
int rkfdNodeGetLinks(rkfdNode *n, int flags, double *R, double *p, double *v, double *com, double *comvel);
/* rkfdBatchSetJacobianSites on every device (the sites are replicated, like the model; nothing is changed on any device when the
 * list is refused); rkfdBatchUpdateJacobians( flags ) on every device's own thread and stream, then host arrays over ALL instances
 * in instance order (shapes as rkfdBatchGetJacobians with batch = total; the pointer of a quantity `flags` does not select must be NULL) */
int rkfdNodeSetJacobianSites(rkfdNode *n, int nsite, const int *link, const double *point);
int rkfdNodeGetJacobians(rkfdNode *n, int flags, double *J, double *Jcom);
/* rkfdBatchUpdateDynamics( flags ) on every device's own thread and stream, then host arrays over ALL instances in instance order
 * (shapes as rkfdBatchGetDynamics with batch = total; pointers of quantities `flags` does not select must be NULL) */
int rkfdNodeGetDynamics(rkfdNode *n, int flags, double *M, double *h, double *g);
/* rkfdBatchUpdateContactForces( flags ) on every device's own thread and stream, then host arrays over ALL instances in instance
 * order (shapes as rkfdBatchGetContactForces with batch = total; pointers of quantities `flags` does not select must be NULL) */
int rkfdNodeGetContactForces(rkfdNode *n, int flags, double *point, double *wrench, int *count, double *genf);
/* one ncclAllGather of the final {dis, vel}: afterwards every device holds all `total` final states (rkfdNodeGatherDev: on
 * device k, [ndev][mx][2 ndof] doubles - block j = shard j's instances, dis | vel per instance, padded to the largest shard mx),
 * and dis / vel ([total][ndof], either may be NULL) receive them on the host in instance order */
int rkfdNodeGather(rkfdNode *n, double *dis, double *vel);
const double *rkfdNodeGatherDev(const rkfdNode *n, int k, int *mx);

#ifdef __cplusplus
}
#endif
#endif
