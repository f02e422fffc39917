#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is opened with dlopen when a communicator is first asked for
#include <cstring>

#include "oh_handle.h"

// ---------------------------------------------------------------------------------------------------------------------------
// Multi-GPU: one process per GPU, instances sharded by the host, no data-path collective.  The single exchange of a job is the
// broadcast of the URDF-derived constants from one rank; the library owns the RCCL communicator for it (and for the
// barrier / MAX / SUM reductions a benchmark harness needs), so a ctypes host needs no other GPU runtime.  librccl is opened on first
// use: single-GPU processes never load it.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;  // optional (oh_comm_allgather)
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;     // optional
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;  // optional
};
RcclApi g_rccl;
ncclComm_t g_comm = nullptr;
int g_comm_rank = -1, g_comm_world = 0, g_comm_device = 0;
hipStream_t g_comm_stream = nullptr;
double* g_comm_scratch = nullptr;  // device, 2 doubles

int rccl_load() {
  if (g_rccl.lib) return OH_OK;
  void* lib = nullptr;
  for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
    lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
    if (lib) break;
  }
  if (!lib) return fail(OH_ERR_HIP, std::string("oh_comm: cannot open librccl: ") + dlerror());
  RcclApi a;
  a.lib = lib;
  a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
  a.CommInitRank = (decltype(a.CommInitRank))dlsym(lib, "ncclCommInitRank");
  a.CommDestroy = (decltype(a.CommDestroy))dlsym(lib, "ncclCommDestroy");
  a.Broadcast = (decltype(a.Broadcast))dlsym(lib, "ncclBroadcast");
  a.AllReduce = (decltype(a.AllReduce))dlsym(lib, "ncclAllReduce");
  a.AllGather = (decltype(a.AllGather))dlsym(lib, "ncclAllGather");
  a.GetErrorString = (decltype(a.GetErrorString))dlsym(lib, "ncclGetErrorString");
  a.CommCount = (decltype(a.CommCount))dlsym(lib, "ncclCommCount");
  a.CommUserRank = (decltype(a.CommUserRank))dlsym(lib, "ncclCommUserRank");
  if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.Broadcast || !a.AllReduce || !a.GetErrorString) {
    dlclose(lib);
    return fail(OH_ERR_HIP, "oh_comm: librccl lacks an expected symbol");
  }
  g_rccl = a;
  return OH_OK;
}
int rccl_fail(const char* what, ncclResult_t r) { return fail(OH_ERR_HIP, std::string(what) + ": " + g_rccl.GetErrorString(r)); }
#define RCCLCHK(expr)                                  \
  do {                                                 \
    ncclResult_t _r = (expr);                          \
    if (_r != ncclSuccess) return rccl_fail(#expr, _r); \
  } while (0)
}  // namespace

extern "C" int oh_comm_unique_id(char* id) {
  if (!id) return fail(OH_ERR_INVALID, "oh_comm_unique_id: null");
  static_assert(OH_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");
  if (const int rc = rccl_load()) return rc;
  ncclUniqueId u;
  RCCLCHK(g_rccl.GetUniqueId(&u));
  memcpy(id, u.internal, OH_COMM_ID_BYTES);
  return OH_OK;
}

extern "C" int oh_comm_init(int rank, int world, const char* id) {
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(OH_ERR_INVALID, "oh_comm_init: bad rank / world / id");
  if (g_comm) return fail(OH_ERR_STATE, "oh_comm_init: this process already holds a communicator");
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) return fail(OH_ERR_HIP, "oh_comm_init: no HIP device available (this library has no CPU path)");
  if (const int rc = rccl_load()) return rc;
  HIPCHK(hipGetDevice(&g_comm_device));  // the device selected with oh_set_device
  ncclUniqueId u;
  memcpy(u.internal, id, OH_COMM_ID_BYTES);
  HIPCHK(hipStreamCreate(&g_comm_stream));
  // (oh_chain-sized: the broadcast of the constants lands here first and is validated before a handle adopts it)
  if (hipMalloc((void**)&g_comm_scratch, 2 * sizeof(double) + sizeof(oh_chain)) != hipSuccess) {
    hipStreamDestroy(g_comm_stream);
    g_comm_stream = nullptr;
    return fail(OH_ERR_HIP, "oh_comm_init: scratch allocation failed");
  }
  const ncclResult_t ir = g_rccl.CommInitRank(&g_comm, world, u, rank);
  if (ir != ncclSuccess) {  // a retry must not leak the stream and the scratch
    g_comm = nullptr;
    hipFree(g_comm_scratch);
    g_comm_scratch = nullptr;
    hipStreamDestroy(g_comm_stream);
    g_comm_stream = nullptr;
    return rccl_fail("ncclCommInitRank", ir);
  }
  g_comm_rank = rank;
  g_comm_world = world;
  return OH_OK;
}

extern "C" int oh_comm_destroy(void) {
  if (!g_comm) return OH_OK;
  hipSetDevice(g_comm_device);
  hipStreamSynchronize(g_comm_stream);
  g_rccl.CommDestroy(g_comm);
  g_comm = nullptr;
  hipFree(g_comm_scratch);
  g_comm_scratch = nullptr;
  hipStreamDestroy(g_comm_stream);
  g_comm_stream = nullptr;
  g_comm_rank = -1;
  g_comm_world = 0;
  return OH_OK;
}

static int comm_allreduce(double* value, ncclRedOp_t op, const char* who) {
  if (!value) return fail(OH_ERR_INVALID, std::string(who) + ": null");
  if (!g_comm) return fail(OH_ERR_STATE, std::string(who) + ": call oh_comm_init first");
  HIPCHK(hipSetDevice(g_comm_device));
  HIPCHK(hipMemcpyAsync(g_comm_scratch, value, sizeof(double), hipMemcpyHostToDevice, g_comm_stream));
  RCCLCHK(g_rccl.AllReduce(g_comm_scratch, g_comm_scratch + 1, 1, ncclFloat64, op, g_comm, g_comm_stream));
  HIPCHK(hipMemcpyAsync(value, g_comm_scratch + 1, sizeof(double), hipMemcpyDeviceToHost, g_comm_stream));
  HIPCHK(hipStreamSynchronize(g_comm_stream));
  return OH_OK;
}
extern "C" int oh_comm_allreduce_max(double* value) { return comm_allreduce(value, ncclMax, "oh_comm_allreduce_max"); }
extern "C" int oh_comm_allreduce_sum(double* value) { return comm_allreduce(value, ncclSum, "oh_comm_allreduce_sum"); }
extern "C" int oh_comm_barrier(void) {
  double one = 1.0;
  return comm_allreduce(&one, ncclSum, "oh_comm_barrier");
}

extern "C" int oh_comm_broadcast_constants(oh_handle* h, int root) {
  if (!h) return fail(OH_ERR_INVALID, "oh_comm_broadcast_constants: null handle");
  if (!g_comm) return fail(OH_ERR_STATE, "oh_comm_broadcast_constants: call oh_comm_init first");
  if (root < 0 || root >= g_comm_world) return fail(OH_ERR_INVALID, "oh_comm_broadcast_constants: bad root");
  if (!h->d_chain) return fail(OH_ERR_STATE, "oh_comm_broadcast_constants: this handle takes no kinematic constants");
  if (g_comm_rank == root && !h->have_chain) return fail(OH_ERR_STATE, "oh_comm_broadcast_constants: the root must call oh_set_constants first");
  HIPCHK(hipSetDevice(h->device));
  // one ncclBroadcast of the oh_chain block (2952 B) on the handle's stream: out of the root's constants buffer, into a scratch block on the
  // other ranks -- a chain this handle rejects (wrong ndof, unsupported joint) must not have replaced its constants already
  unsigned char* const land = (unsigned char*)(g_comm_scratch + 2);
  RCCLCHK(g_rccl.Broadcast(h->d_chain, g_comm_rank == root ? (void*)h->d_chain : (void*)land, sizeof(oh_chain), ncclUint8, root, g_comm, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (g_comm_rank != root) {
    oh_chain tmp;
    HIPCHK(hipMemcpy(&tmp, land, sizeof(oh_chain), hipMemcpyDeviceToHost));
    if (const int rc = validate_chain(h, tmp)) return rc;
    HIPCHK(hipMemcpy(h->d_chain, land, sizeof(oh_chain), hipMemcpyDeviceToDevice));
    adopt_chain(h, tmp);
  }
  return OH_OK;
}

// The optional gather of SURVEY 8(e): every rank contributes `bytes` bytes of a device buffer (objectives, statuses, or whole solutions of its shard) and
// receives all ranks' blocks in rank order -- one ncclAllGather over xGMI on the communicator's stream, after the solves; never part of the data path.
extern "C" int oh_comm_allgather(const void* d_send, void* d_recv, size_t bytes) {
  if (!d_send || !d_recv || bytes == 0) return fail(OH_ERR_INVALID, "oh_comm_allgather: null buffer or zero size");
  if (!g_comm) return fail(OH_ERR_STATE, "oh_comm_allgather: call oh_comm_init first");
  if (!g_rccl.AllGather) return fail(OH_ERR_HIP, "oh_comm_allgather: librccl lacks ncclAllGather");
  HIPCHK(hipSetDevice(g_comm_device));
  RCCLCHK(g_rccl.AllGather(d_send, d_recv, bytes, ncclUint8, g_comm, g_comm_stream));
  HIPCHK(hipStreamSynchronize(g_comm_stream));
  return OH_OK;
}

// world size and rank as RCCL sees them (a harness prints them to prove the communicator spans the job)
extern "C" int oh_comm_info(int* rank, int* world) {
  if (!g_comm) return fail(OH_ERR_STATE, "oh_comm_info: call oh_comm_init first");
  int r = -1, w = 0;
  if (g_rccl.CommUserRank) RCCLCHK(g_rccl.CommUserRank(g_comm, &r)); else r = g_comm_rank;
  if (g_rccl.CommCount) RCCLCHK(g_rccl.CommCount(g_comm, &w)); else w = g_comm_world;
  if (rank) *rank = r;
  if (world) *world = w;
  return OH_OK;
}
