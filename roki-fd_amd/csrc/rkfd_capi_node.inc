/* rkfd_capi_node.inc - part of rkfd_capi.hip (included at its end): the NODE level of the C ABI (include/rkfd_hip.h, rkfdNode*).
 *
 * One process drives all the GPUs of a node: the instances of a batch are independent (one rkFD never references another,
 * SURVEY 8e), so device k simulates the contiguous block shard k of `total` instances - model constants replicated, NO per-step
 * communication - with one host thread and one HIP stream per device, and the only collective is one all-gather of the final
 * {dis, vel} per rollout through RCCL (ncclAllGather over xGMI; librccl is bound at run time, the library does not link it).
 * The reference has no counterpart: it is single-threaded C on one core.  Host code stays C-callable: plain pointers and sizes.
 */
#include <rccl/rccl.h>

struct rkfdRccl {
  void *h;
  ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *);
  ncclResult_t (*CommDestroy)(ncclComm_t);
  ncclResult_t (*GroupStart)(void);
  ncclResult_t (*GroupEnd)(void);
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t);
  const char *(*GetErrorString)(ncclResult_t);
};
/* binds librccl once per process: RKFD_RCCL_LIB names the file, else the soname (a host program that has already loaded an RCCL -
 * PyTorch bundles one - is served by that copy), else the ROCm directory this library was built against */
static const rkfdRccl *rccl_api(void)
{
  static rkfdRccl api;
  static int state = 0;      /* 0 untried, 1 ok, -1 failed */
  static pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
  pthread_mutex_lock( &mu );
  if( state == 0 ){
    const char *env = getenv( "RKFD_RCCL_LIB" );
    const char *cand[] = { env, "librccl.so.1", "librccl.so", RKFD_ROCM_LIBDIR "/librccl.so.1", NULL };
    void *h = NULL;
    for( int i=0; i<4 && !h; i++ ) if( cand[i] ) h = dlopen( cand[i], RTLD_NOW | RTLD_LOCAL );
    state = -1;
    if( !h ) SETERR( "rkfdNode: librccl could not be loaded (%s); set RKFD_RCCL_LIB", dlerror() );
    else {
      api.h = h;
      api.CommInitAll = (ncclResult_t (*)(ncclComm_t *, int, const int *))dlsym( h, "ncclCommInitAll" );
      api.CommDestroy = (ncclResult_t (*)(ncclComm_t))dlsym( h, "ncclCommDestroy" );
      api.GroupStart = (ncclResult_t (*)(void))dlsym( h, "ncclGroupStart" );
      api.GroupEnd = (ncclResult_t (*)(void))dlsym( h, "ncclGroupEnd" );
      api.AllGather = (ncclResult_t (*)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t))dlsym( h, "ncclAllGather" );
      api.GetErrorString = (const char *(*)(ncclResult_t))dlsym( h, "ncclGetErrorString" );
      if( api.CommInitAll && api.CommDestroy && api.GroupStart && api.GroupEnd && api.AllGather && api.GetErrorString ) state = 1;
      else SETERR( "rkfdNode: librccl lacks an expected symbol" );
    }
  }
  pthread_mutex_unlock( &mu );
  return state == 1 ? &api : NULL;
}

enum { NODE_CMD_NONE = 0, NODE_CMD_INIT, NODE_CMD_UPDATE, NODE_CMD_SPECIALIZE, NODE_CMD_SPLIT, NODE_CMD_STEPS_PER_LAUNCH, NODE_CMD_TUNE, NODE_CMD_STATUS, NODE_CMD_SNAPSHOT, NODE_CMD_RESTORE, NODE_CMD_PACK, NODE_CMD_UPDATE_CTRL, NODE_CMD_LINKS, NODE_CMD_RESET, NODE_CMD_JAC, NODE_CMD_DYN, NODE_CMD_CF, NODE_CMD_QUIT };

struct rkfdNode;
struct rkfdNodeWorker {
  rkfdNode *node;
  int k;                 /* index of the device in the node */
  pthread_t th;
  int started;
  int result;            /* of the last command */
  char err[512];
};
struct rkfdNode {
  int ndev, total, ndof, nlink, ncand, mx;     /* mx: instances of the largest shard (the all-gather wants equal blocks) */
  std::vector<int> dev, lo, hi;
  std::vector<rkfdBatch *> b;
  std::vector<hipStream_t> st;
  std::vector<rkfdNodeWorker> w;
  /* command hand-off: the caller publishes (cmd, arg) under mu and bumps seq; every worker runs it on its device and counts itself done */
  pthread_mutex_t mu;
  pthread_cond_t cv_cmd, cv_done;
  int cmd, arg, seq, done;
  const double *ctrl;        /* NODE_CMD_UPDATE_CTRL: the caller's host schedule [total][arg][nlink] */
  /* gather */
  std::vector<ncclComm_t> comm;
  int have_comm;
  std::vector<double *> d_send, d_recv;        /* [mx][2 ndof] and [ndev][mx][2 ndof] per device */
};

static int node_run_on(rkfdNode *n, int k, int cmd, int arg)
{
  rkfdBatch *b = n->b[k];
  switch( cmd ){
  case NODE_CMD_INIT:       return rkfdBatchUpdateInit( b, n->st[k] );
  case NODE_CMD_UPDATE:     return rkfdBatchUpdate( b, arg, n->st[k] );
  case NODE_CMD_UPDATE_CTRL: return rkfdBatchUpdateControlled( b, arg, n->ctrl + (size_t)n->lo[k]*arg*n->nlink, n->st[k] );
  case NODE_CMD_LINKS:      return rkfdBatchUpdateLinks( b, arg, n->st[k] );
  case NODE_CMD_JAC:        return rkfdBatchUpdateJacobians( b, arg, n->st[k] );
  case NODE_CMD_DYN:        return rkfdBatchUpdateDynamics( b, arg, n->st[k] );
  case NODE_CMD_CF:         return rkfdBatchUpdateContactForces( b, arg, n->st[k] );
  case NODE_CMD_RESET:      return reset_launch( b, NULL, n->st[k], "rkfdNodeReset" );      /* (rkfdNodeReset has staged the shard's slot values) */
  case NODE_CMD_SPECIALIZE: return rkfdBatchSpecialize( b );
  case NODE_CMD_SPLIT:      return rkfdBatchSetSplit( b, arg );
  case NODE_CMD_STEPS_PER_LAUNCH: return rkfdBatchSetStepsPerLaunch( b, arg );
  case NODE_CMD_TUNE: {      /* (every device measures for itself: the mappings give the same bits, so devices may differ) */
    const int r = rkfdBatchTuneInstancesPerWave( b, arg, NULL );
    return r < 0 ? r : 0;
  }
  case NODE_CMD_STATUS:     return rkfdBatchStatus( b, n->st[k] );
  case NODE_CMD_SNAPSHOT:   return rkfdBatchSnapshot( b );
  case NODE_CMD_RESTORE:    return rkfdBatchRestore( b, n->st[k] );
  case NODE_CMD_PACK: {
    /* this device's final {dis, vel}, instance-major [nloc][2 ndof], into the head of its send block (stream-ordered after the steps) */
    const int nloc = n->hi[k] - n->lo[k];
    const size_t row = sizeof(double)*n->ndof;
    if( rkfdBatchJoin( b, n->st[k] ) < 0 ) return -1;
    HIPCHK( hipSetDevice( n->dev[k] ), -1 );
    if( nloc > 0 && n->ndof > 0 ){
      HIPCHK( hipMemcpy2DAsync( n->d_send[k], 2*row, rkfdBatchDevDis( b ), row, row, (size_t)nloc, hipMemcpyDeviceToDevice, n->st[k] ), -1 );
      HIPCHK( hipMemcpy2DAsync( (char *)n->d_send[k] + row, 2*row, rkfdBatchDevVel( b ), row, row, (size_t)nloc, hipMemcpyDeviceToDevice, n->st[k] ), -1 );
    }
    return 0;
  }
  default: return 0;
  }
}
static void *node_worker(void *arg)
{
  rkfdNodeWorker *w = (rkfdNodeWorker *)arg;
  rkfdNode *n = w->node;
  int seen = 0;
  for(;;){
    pthread_mutex_lock( &n->mu );
    while( n->seq == seen ) pthread_cond_wait( &n->cv_cmd, &n->mu );
    seen = n->seq;
    const int cmd = n->cmd, a = n->arg;
    pthread_mutex_unlock( &n->mu );
    if( cmd != NODE_CMD_QUIT ){
      w->result = node_run_on( n, w->k, cmd, a );
      if( w->result != 0 ) snprintf( w->err, sizeof(w->err), "device %d: %s", n->dev[w->k], g_err );
    }
    pthread_mutex_lock( &n->mu );
    n->done++;
    pthread_cond_signal( &n->cv_done );
    pthread_mutex_unlock( &n->mu );
    if( cmd == NODE_CMD_QUIT ) break;
  }
  return NULL;
}
/* runs cmd on every device, each in its own host thread; returns the worst result (the STATUS command: the largest positive
 * status unless a device failed) with that device's message as the caller's last error */
static int node_all(rkfdNode *n, int cmd, int arg)
{
  pthread_mutex_lock( &n->mu );
  n->cmd = cmd; n->arg = arg; n->done = 0; n->seq++;
  pthread_cond_broadcast( &n->cv_cmd );
  while( n->done < n->ndev ) pthread_cond_wait( &n->cv_done, &n->mu );
  pthread_mutex_unlock( &n->mu );
  int r = 0, which = -1;
  for( int k=0; k<n->ndev; k++ ){
    const int rk = n->w[k].result;
    if( rk < 0 ){ r = rk; which = k; break; }
    if( rk > r ){ r = rk; which = k; }
  }
  if( which >= 0 ) SETERR( "%s", n->w[which].err );
  return r;
}

extern "C" void rkfdNodeDestroy(rkfdNode *n)
{
  if( !n ) return;
  int started = 0;
  for( size_t k=0; k<n->w.size(); k++ ) started += n->w[k].started;
  if( started > 0 ){
    pthread_mutex_lock( &n->mu );
    n->cmd = NODE_CMD_QUIT; n->done = 0; n->seq++;
    pthread_cond_broadcast( &n->cv_cmd );
    pthread_mutex_unlock( &n->mu );
    for( size_t k=0; k<n->w.size(); k++ ) if( n->w[k].started ) pthread_join( n->w[k].th, NULL );
  }
  if( n->have_comm ){
    const rkfdRccl *rc = rccl_api();
    if( rc ) for( size_t k=0; k<n->comm.size(); k++ ) rc->CommDestroy( n->comm[k] );
  }
  for( size_t k=0; k<n->b.size(); k++ ){
    if( k < n->dev.size() ) (void)hipSetDevice( n->dev[k] );
    if( k < n->d_send.size() && n->d_send[k] ) (void)hipFree( n->d_send[k] );
    if( k < n->d_recv.size() && n->d_recv[k] ) (void)hipFree( n->d_recv[k] );
    if( k < n->st.size() && n->st[k] ) (void)hipStreamDestroy( n->st[k] );
    if( n->b[k] ) rkfdBatchDestroy( n->b[k] );
  }
  pthread_mutex_destroy( &n->mu ); pthread_cond_destroy( &n->cv_cmd ); pthread_cond_destroy( &n->cv_done );
  delete n;
}

extern "C" rkfdNode *rkfdNodeCreate(const rkfdModel *m, int total, int max_rigid, int ndev, const int *devices)
{
  if( !m || total < 1 ){ SETERR( "rkfdNodeCreate: null model or empty batch" ); return NULL; }
  int have = 0;
  if( hipGetDeviceCount( &have ) != hipSuccess || have < 1 ){ SETERR( "rkfdNodeCreate: no HIP device available (the MI355X path has no CPU fallback)" ); return NULL; }
  if( ndev <= 0 ) ndev = have;
  if( ndev > total ) ndev = total;
  rkfdNode *n = new rkfdNode();
  n->ndev = ndev; n->total = total; n->ndof = m->ndof; n->nlink = m->nlink; n->ncand = m->ncand; n->have_comm = 0;
  n->cmd = NODE_CMD_NONE; n->arg = 0; n->seq = 0; n->done = 0; n->ctrl = NULL;
  pthread_mutex_init( &n->mu, NULL ); pthread_cond_init( &n->cv_cmd, NULL ); pthread_cond_init( &n->cv_done, NULL );
  n->dev.resize( ndev ); n->lo.resize( ndev ); n->hi.resize( ndev );
  n->b.assign( ndev, NULL ); n->st.assign( ndev, NULL ); n->d_send.assign( ndev, NULL ); n->d_recv.assign( ndev, NULL );
  n->w.resize( ndev );
  n->mx = 0;
  for( int k=0; k<ndev; k++ ){
    n->dev[k] = devices ? devices[k] : k;
    if( n->dev[k] < 0 || n->dev[k] >= have ){ SETERR( "rkfdNodeCreate: device %d is not one of the %d visible", n->dev[k], have ); rkfdNodeDestroy( n ); return NULL; }
    /* contiguous blocks, remainders to the low devices (the partition of roki-fd_amd/sharding.py: shard_range) */
    const int base = total/ndev, rem = total%ndev;
    n->lo[k] = k*base + ( k < rem ? k : rem );
    n->hi[k] = n->lo[k] + base + ( k < rem ? 1 : 0 );
    if( n->hi[k] - n->lo[k] > n->mx ) n->mx = n->hi[k] - n->lo[k];
    n->w[k].node = n; n->w[k].k = k; n->w[k].started = 0; n->w[k].result = 0; n->w[k].err[0] = 0;
  }
  for( int k=0; k<ndev; k++ ){
    n->b[k] = rkfdBatchCreate( m, n->hi[k] - n->lo[k], n->dev[k], max_rigid );
    if( !n->b[k] ){ rkfdNodeDestroy( n ); return NULL; }
    const size_t blk = sizeof(double)*2*( n->ndof > 0 ? n->ndof : 1 )*(size_t)n->mx;
    if( hipSetDevice( n->dev[k] ) != hipSuccess || hipStreamCreateWithFlags( &n->st[k], hipStreamNonBlocking ) != hipSuccess ||
        hipMalloc( (void **)&n->d_send[k], blk ) != hipSuccess || hipMalloc( (void **)&n->d_recv[k], blk*ndev ) != hipSuccess ||
        hipMemset( n->d_send[k], 0, blk ) != hipSuccess ){
      SETERR( "rkfdNodeCreate: stream / gather buffers on device %d failed", n->dev[k] ); rkfdNodeDestroy( n ); return NULL;
    }
  }
  for( int k=0; k<ndev; k++ ){
    if( pthread_create( &n->w[k].th, NULL, node_worker, &n->w[k] ) != 0 ){ SETERR( "rkfdNodeCreate: pthread_create failed" ); rkfdNodeDestroy( n ); return NULL; }
    n->w[k].started = 1;
  }
  return n;
}

extern "C" int rkfdNodeDevices(const rkfdNode *n){ return n ? n->ndev : 0; }
extern "C" int rkfdNodeSize(const rkfdNode *n){ return n ? n->total : 0; }
extern "C" int rkfdNodeShard(const rkfdNode *n, int k, int *device, int *lo, int *hi)
{
  if( !n || k < 0 || k >= n->ndev ){ SETERR( "rkfdNodeShard: no such shard" ); return -1; }
  if( device ) *device = n->dev[k];
  if( lo ) *lo = n->lo[k];
  if( hi ) *hi = n->hi[k];
  return 0;
}
extern "C" rkfdBatch *rkfdNodeBatch(rkfdNode *n, int k){ return ( n && k >= 0 && k < n->ndev ) ? n->b[k] : NULL; }

extern "C" int rkfdNodeSetState(rkfdNode *n, const double *dis, const double *vel)
{
  if( !n || !dis || !vel ){ SETERR( "rkfdNodeSetState: null argument" ); return -1; }
  for( int k=0; k<n->ndev; k++ )
    if( rkfdBatchSetState( n->b[k], dis + (size_t)n->lo[k]*n->ndof, vel + (size_t)n->lo[k]*n->ndof ) < 0 ) return -1;
  return 0;
}
/* per-instance parameters over all instances: every shard is checked before any is changed */
extern "C" int rkfdNodeSetParam(rkfdNode *n, int which, const double *values)
{
  if( !n ){ SETERR( "rkfdNodeSetParam: null node" ); return -1; }
  for( int k=0; k<n->ndev; k++ ){
    const int w = rkfdBatchParamWidth( n->b[k], which );
    if( par_check( n->b[k], which, values && w > 0 ? values + (size_t)n->lo[k]*w : values ) < 0 ) return -1;
  }
  for( int k=0; k<n->ndev; k++ ){
    const int w = rkfdBatchParamWidth( n->b[k], which );
    if( rkfdBatchSetParam( n->b[k], which, values ? values + (size_t)n->lo[k]*w : NULL ) < 0 ) return -1;
  }
  return 0;
}
extern "C" int rkfdNodeClearParams(rkfdNode *n)
{
  if( !n ){ SETERR( "rkfdNodeClearParams: null node" ); return -1; }
  for( int k=0; k<n->ndev; k++ ) if( rkfdBatchClearParams( n->b[k] ) < 0 ) return -1;
  return 0;
}
extern "C" int rkfdNodeSetMotorInput(rkfdNode *n, const double *input)
{
  if( !n || !input ){ SETERR( "rkfdNodeSetMotorInput: null argument" ); return -1; }
  for( int k=0; k<n->ndev; k++ ) if( rkfdBatchSetMotorInput( n->b[k], input + (size_t)n->lo[k]*n->nlink ) < 0 ) return -1;
  return 0;
}
extern "C" int rkfdNodeGetState(rkfdNode *n, double *dis, double *vel, double *acc)
{
  if( !n ){ SETERR( "null node" ); return -1; }
  for( int k=0; k<n->ndev; k++ ){
    const size_t o = (size_t)n->lo[k]*n->ndof;
    if( rkfdBatchJoin( n->b[k], n->st[k] ) < 0 ) return -1;
    HIPCHK( hipSetDevice( n->dev[k] ), -1 );
    HIPCHK( hipStreamSynchronize( n->st[k] ), -1 );
    if( rkfdBatchGetState( n->b[k], dis ? dis+o : NULL, vel ? vel+o : NULL, acc ? acc+o : NULL ) < 0 ) return -1;
  }
  return 0;
}
extern "C" int rkfdNodeSpecialize(rkfdNode *n){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_SPECIALIZE, 0 ); }
extern "C" int rkfdNodeSetSplit(rkfdNode *n, int nsplit){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_SPLIT, nsplit ); }
extern "C" int rkfdNodeSetStepsPerLaunch(rkfdNode *n, int steps){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_STEPS_PER_LAUNCH, steps ); }
extern "C" int rkfdNodeTuneInstancesPerWave(rkfdNode *n, int nsteps){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_TUNE, nsteps ); }
extern "C" int rkfdNodeUpdateInit(rkfdNode *n){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_INIT, 0 ); }
extern "C" int rkfdNodeUpdate(rkfdNode *n, int nsteps){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_UPDATE, nsteps ); }
extern "C" int rkfdNodeSnapshot(rkfdNode *n){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_SNAPSHOT, 0 ); }
extern "C" int rkfdNodeRestore(rkfdNode *n){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_RESTORE, 0 ); }
extern "C" int rkfdNodeStatus(rkfdNode *n){ if( !n ){ SETERR( "null node" ); return -1; } return node_all( n, NODE_CMD_STATUS, 0 ); }
extern "C" int rkfdNodeUpdateControlled(rkfdNode *n, int nsteps, const double *u)
{
  if( !n || !u || nsteps < 1 ){ SETERR( "rkfdNodeUpdateControlled: %s", !n ? "null node" : !u ? "null schedule" : "nsteps must be >= 1" ); return -1; }
  n->ctrl = u;      /* (read by the workers only while node_all waits for them: every copy out of u is made before it returns) */
  const int r = node_all( n, NODE_CMD_UPDATE_CTRL, nsteps );
  n->ctrl = NULL;
  return r;
}

/* ---- per-instance reset over all instances: the bank is replicated like the model, the slot values are sharded like the state ---- */
extern "C" int rkfdNodeBankReserve(rkfdNode *n, int nslots)
{
  if( !n ){ SETERR( "rkfdNodeBankReserve: null node" ); return -1; }
  if( nslots < 0 ){ SETERR( "rkfdNodeBankReserve: nslots must be >= 0 (got %d)", nslots ); return -1; }
  for( int k=0; k<n->ndev; k++ ) if( rkfdBatchBankReserve( n->b[k], nslots ) < 0 ) return -1;
  return 0;
}
/* rows slot .. slot+count-1 of EVERY device's bank <- the live state of the instances first .. first+count-1 (global indices): read
 * from the shards that own them, through the host */
extern "C" int rkfdNodeBankStore(rkfdNode *n, int slot, int first, int count)
{
  if( !n ){ SETERR( "rkfdNodeBankStore: null node" ); return -1; }
  if( count < 1 || first < 0 || (long long)first + count > n->total ){ SETERR( "rkfdNodeBankStore: instances %d .. %d are not within the %d of the node", first, first+count-1, n->total ); return -1; }
  for( int k=0; k<n->ndev; k++ ){
    const int have = rkfdBatchBankSize( n->b[k] );
    if( slot < 0 || (long long)slot + count > have ){ SETERR( "rkfdNodeBankStore: rows %d .. %d are not within the bank of %d (rkfdNodeBankReserve)", slot, slot+count-1, have ); return -1; }
  }
  for( int k=0; k<n->ndev; k++ ){
    const int lo = first > n->lo[k] ? first : n->lo[k], hi = first + count < n->hi[k] ? first + count : n->hi[k];
    if( hi <= lo ) continue;
    std::vector<char> buf( rkfd_reset_row_bytes( n->b[k]->reset, hi-lo ) + 8 );
    if( bank_rows_get( n->b[k], lo - n->lo[k], hi-lo, buf.data() ) < 0 ) return -1;
    for( int j=0; j<n->ndev; j++ ) if( bank_rows_put( n->b[j], slot + ( lo-first ), hi-lo, buf.data() ) < 0 ) return -1;
  }
  return 0;
}
/* slots[total] on the host, sharded like rkfdNodeSetState: every shard's block goes into its batch's pinned staging first - a
 * refusal there leaves every device as it was -, then every device's own thread issues its reset on its own stream */
extern "C" int rkfdNodeReset(rkfdNode *n, const int *slots)
{
  if( !n || !slots ){ SETERR( "rkfdNodeReset: %s", !n ? "null node" : "null slots" ); return -1; }
  for( int k=0; k<n->ndev; k++ ) if( reset_stage( n->b[k], slots + n->lo[k], "rkfdNodeReset" ) < 0 ) return -1;
  return node_all( n, NODE_CMD_RESET, 0 );
}

/* the task-space read-out over all instances: rkfdBatchUpdateLinks on every device's own thread and stream, then the host arrays
 * in instance order (the pointers of quantities `flags` does not select must be NULL) */
extern "C" int rkfdNodeGetLinks(rkfdNode *n, int flags, double *R, double *p, double *v, double *com, double *comvel)
{
  if( !n ){ SETERR( "rkfdNodeGetLinks: null node" ); return -1; }
  if( node_all( n, NODE_CMD_LINKS, flags ) < 0 ) return -1;
  for( int k=0; k<n->ndev; k++ ){
    const size_t lo = (size_t)n->lo[k], nl = (size_t)n->nlink, nc = (size_t)rkfdBatchChainNum( n->b[k] );
    if( rkfdBatchGetLinks( n->b[k], R ? R + lo*nl*9 : NULL, p ? p + lo*nl*3 : NULL, v ? v + lo*nl*6 : NULL,
                           com ? com + lo*nc*3 : NULL, comvel ? comvel + lo*nc*3 : NULL ) < 0 ) return -1;
  }
  return 0;
}

/* the task-space Jacobians over all instances: the sites are the same on every device (replicated, like the model); nothing is
 * changed on any device when the list is refused (it is checked against the model before the first device takes it) */
extern "C" int rkfdNodeSetJacobianSites(rkfdNode *n, int nsite, const int *link, const double *point)
{
  if( !n ){ SETERR( "rkfdNodeSetJacobianSites: null node" ); return -1; }
  char err[400] = "";
  if( rkfd_jac_check_sites( n->nlink, nsite, link, point, err, sizeof(err) ) < 0 ){ SETERR( "rkfdNodeSetJacobianSites: %s", err ); return -1; }
  for( int k=0; k<n->ndev; k++ ) if( rkfdBatchSetJacobianSites( n->b[k], nsite, link, point ) < 0 ) return -1;
  return 0;
}
/* rkfdBatchUpdateJacobians( flags ) on every device's own thread and stream, then the host arrays in instance order (the pointer of
 * a quantity `flags` does not select must be NULL) */
extern "C" int rkfdNodeGetJacobians(rkfdNode *n, int flags, double *J, double *Jcom)
{
  if( !n ){ SETERR( "rkfdNodeGetJacobians: null node" ); return -1; }
  if( node_all( n, NODE_CMD_JAC, flags ) < 0 ) return -1;
  for( int k=0; k<n->ndev; k++ ){
    const size_t lo = (size_t)n->lo[k], nd = (size_t)n->ndof, nc = (size_t)rkfdBatchChainNum( n->b[k] ), ns = (size_t)rkfdBatchJacobianSiteNum( n->b[k] );
    if( rkfdBatchGetJacobians( n->b[k], J ? J + lo*ns*6*nd : NULL, Jcom ? Jcom + lo*nc*3*nd : NULL ) < 0 ) return -1;
  }
  return 0;
}
/* rkfdBatchUpdateDynamics( flags ) on every device's own thread and stream, then the host arrays in instance order (the pointer of
 * a quantity `flags` does not select must be NULL) */
extern "C" int rkfdNodeGetDynamics(rkfdNode *n, int flags, double *M, double *h, double *g)
{
  if( !n ){ SETERR( "rkfdNodeGetDynamics: null node" ); return -1; }
  if( node_all( n, NODE_CMD_DYN, flags ) < 0 ) return -1;
  for( int k=0; k<n->ndev; k++ ){
    const size_t lo = (size_t)n->lo[k], nd = (size_t)n->ndof;
    if( rkfdBatchGetDynamics( n->b[k], M ? M + lo*nd*nd : NULL, h ? h + lo*nd : NULL, g ? g + lo*nd : NULL ) < 0 ) return -1;
  }
  return 0;
}
/* rkfdBatchUpdateContactForces( flags ) on every device's own thread and stream, then the host arrays in instance order (the
 * pointer of a quantity `flags` does not select must be NULL) */
extern "C" int rkfdNodeGetContactForces(rkfdNode *n, int flags, double *point, double *wrench, int *count, double *genf)
{
  if( !n ){ SETERR( "rkfdNodeGetContactForces: null node" ); return -1; }
  if( node_all( n, NODE_CMD_CF, flags ) < 0 ) return -1;
  for( int k=0; k<n->ndev; k++ ){
    const size_t lo = (size_t)n->lo[k], nd = (size_t)n->ndof, nl = (size_t)n->nlink, nc = (size_t)n->ncand;
    if( rkfdBatchGetContactForces( n->b[k], point ? point + lo*nc*3 : NULL, wrench ? wrench + lo*nl*6 : NULL, count ? count + lo*nl : NULL,
                                   genf ? genf + lo*nd : NULL ) < 0 ) return -1;
  }
  return 0;
}

/* the path's only collective: every device contributes its block of final {dis, vel} ([mx][2 ndof] doubles, its own instances
 * first, padded to the largest shard) to one ncclAllGather; afterwards EVERY device holds the final states of all `total`
 * instances (rkfdNodeGatherDev), and the first device's copy is brought to the host in instance order (dis, vel: [total][ndof],
 * either may be NULL).  Stream-ordered after the steps issued so far; returns when the host copies are complete. */
extern "C" int rkfdNodeGather(rkfdNode *n, double *dis, double *vel)
{
  if( !n ){ SETERR( "null node" ); return -1; }
  const rkfdRccl *rc = rccl_api();
  if( !rc ) return -1;
  if( !n->have_comm ){
    n->comm.resize( n->ndev );
    const ncclResult_t r = rc->CommInitAll( n->comm.data(), n->ndev, n->dev.data() );
    if( r != ncclSuccess ){ SETERR( "rkfdNodeGather: ncclCommInitAll over %d device(s) failed: %s", n->ndev, rc->GetErrorString( r ) ); n->comm.clear(); return -1; }
    n->have_comm = 1;
  }
  if( node_all( n, NODE_CMD_PACK, 0 ) < 0 ) return -1;
  const size_t cnt = (size_t)2*n->ndof*(size_t)n->mx;
  ncclResult_t r = rc->GroupStart();
  for( int k=0; k<n->ndev && r == ncclSuccess; k++ ) r = rc->AllGather( n->d_send[k], n->d_recv[k], cnt, ncclDouble, n->comm[k], n->st[k] );
  const ncclResult_t r2 = rc->GroupEnd();
  if( r != ncclSuccess || r2 != ncclSuccess ){ SETERR( "rkfdNodeGather: ncclAllGather failed: %s", rc->GetErrorString( r != ncclSuccess ? r : r2 ) ); return -1; }
  for( int k=0; k<n->ndev; k++ ){
    HIPCHK( hipSetDevice( n->dev[k] ), -1 );
    HIPCHK( hipStreamSynchronize( n->st[k] ), -1 );
  }
  if( dis || vel ){
    std::vector<double> host( cnt*(size_t)n->ndev );
    HIPCHK( hipSetDevice( n->dev[0] ), -1 );
    HIPCHK( hipMemcpy( host.data(), n->d_recv[0], sizeof(double)*host.size(), hipMemcpyDeviceToHost ), -1 );
    for( int k=0; k<n->ndev; k++ )
      for( int i=n->lo[k]; i<n->hi[k]; i++ ){
        const double *row = &host[cnt*(size_t)k + (size_t)2*n->ndof*( i - n->lo[k] )];
        if( dis ) memcpy( dis + (size_t)i*n->ndof, row, sizeof(double)*n->ndof );
        if( vel ) memcpy( vel + (size_t)i*n->ndof, row + n->ndof, sizeof(double)*n->ndof );
      }
  }
  return 0;
}
/* device pointer (on device k of the node) to the gathered states after rkfdNodeGather: [ndev][mx][2 ndof] doubles, block j holding
 * shard j's instances ( dis | vel per instance ) followed by padding up to mx = the largest shard */
extern "C" const double *rkfdNodeGatherDev(const rkfdNode *n, int k, int *mx)
{
  if( !n || k < 0 || k >= n->ndev ) return NULL;
  if( mx ) *mx = n->mx;
  return n->d_recv[k];
}
