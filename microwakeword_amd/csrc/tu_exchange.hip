// Host-only translation unit of the data-parallel exchange binding (engine.hip.h Exchange): the caller's hook
// (mww_set_allreduce_hook) and the library's own RCCL exchange behind the same hook (mww_allreduce_*).  What a step exchanges,
// and when, is the step's business (mww_lib.hip: exchange_stats, exchange_range, the gradient buckets).
#define MWW_BLOCK_TU 1   // the non-template kernels of the block-kernel headers belong to mww_lib.hip
#include "engine.hip.h"

#include <dlfcn.h>

#include <cstring>

namespace mww {

// RCCL bound at run time (dlopen: the library loads on hosts without RCCL and shares the copy a framework in the same
// process has already loaded); only the five entry points the gradient / statistics exchange needs
struct RcclApi {
  void* so = nullptr;
  struct UniqueId { char internal[128]; };
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;   // optional: mww_allreduce_world
  const char* (*GetErrorString)(int) = nullptr;
};

// ---- RCCL inside the library (mww_allreduce_init).  The exchange the caller's hook performed through
// Python / torch.distributed (two ctypes callbacks, two dispatcher round trips and a pair of cross-stream event waits
// per step: +38 us at W = 1 for the two-bucket schedule in round 2) is issued here, from the launching thread:
//   MWW_EXCHANGE_IN_ORDER  ncclAllReduce on the context's stream itself
//   MWW_EXCHANGE_DEFERRED  event on the context's stream -> the library's side stream waits for it -> ncclAllReduce there
//   MWW_EXCHANGE_FLUSH     the context's stream waits for the side stream's last exchange
struct RcclState {
  RcclApi api;
  void* comm = nullptr;
  hipStream_t side = nullptr;
  hipEvent_t ev_ready = nullptr, ev_done = nullptr;
  mww_ctx* c = nullptr;
  bool deferred = false;
};

namespace {

int rccl_load(RcclApi* a) {
  if (a->so) return MWW_OK;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names) {
    a->so = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (a->so) break;
  }
  if (!a->so) return fail(MWW_ERR_UNSUPPORTED, std::string("librccl.so not found: ") + dlerror());
  a->GetUniqueId = reinterpret_cast<decltype(a->GetUniqueId)>(dlsym(a->so, "ncclGetUniqueId"));
  a->CommInitRank = reinterpret_cast<decltype(a->CommInitRank)>(dlsym(a->so, "ncclCommInitRank"));
  a->AllReduce = reinterpret_cast<decltype(a->AllReduce)>(dlsym(a->so, "ncclAllReduce"));
  a->CommDestroy = reinterpret_cast<decltype(a->CommDestroy)>(dlsym(a->so, "ncclCommDestroy"));
  a->GetErrorString = reinterpret_cast<decltype(a->GetErrorString)>(dlsym(a->so, "ncclGetErrorString"));
  a->CommCount = reinterpret_cast<decltype(a->CommCount)>(dlsym(a->so, "ncclCommCount"));
  if (!a->GetUniqueId || !a->CommInitRank || !a->AllReduce || !a->CommDestroy || !a->GetErrorString)
    return fail(MWW_ERR_UNSUPPORTED, "librccl.so lacks an entry point");
  return MWW_OK;
}

int rccl_exchange(void* user, float* buf, int64_t n, int flags) {
  RcclState* r = static_cast<RcclState*>(user);
  mww_ctx* c = r->c;
  constexpr int kFloat = 7, kSum = 0;   // ncclFloat32, ncclSum (rccl.h)
  if (flags == MWW_EXCHANGE_FLUSH) {
    if (r->deferred) {
      if (hipStreamWaitEvent(c->stream, r->ev_done, 0) != hipSuccess) return -1;
      r->deferred = false;
    }
    return 0;
  }
  hipStream_t st = c->stream;
  if (flags == MWW_EXCHANGE_DEFERRED) {
    if (hipEventRecord(r->ev_ready, c->stream) != hipSuccess) return -1;
    if (hipStreamWaitEvent(r->side, r->ev_ready, 0) != hipSuccess) return -1;
    st = r->side;
  }
  const int e = r->api.AllReduce(buf, buf, (size_t)n, kFloat, kSum, r->comm, st);
  if (e != 0) {
    (void)fail(MWW_ERR_HIP, std::string("ncclAllReduce: ") + r->api.GetErrorString(e));
    return -1;
  }
  if (flags == MWW_EXCHANGE_DEFERRED) {
    if (hipEventRecord(r->ev_done, r->side) != hipSuccess) return -1;
    r->deferred = true;
  }
  return 0;
}

}  // namespace
}  // namespace mww

using namespace mww;

extern "C" {

int mww_set_allreduce_hook(mww_ctx* c, mww_allreduce_fn fn, void* user, int world_size, int sync_bn, int reduce_grads) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  if (fn && world_size < 1) return fail(MWW_ERR_INVALID, "world size must be positive");
  if (fn) MWW_TRY(single_device_only(c, nullptr));
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  Exchange& x = c->xch;
  x.hook = fn;
  x.user = user;
  x.world = fn ? world_size : 1;
  x.sync_bn = fn && sync_bn;
  x.reduce_grads = fn && reduce_grads;
  if (x.sync_bn && !x.sync_buf) {
    int64_t off = 0;
    x.sync_off.clear();
    for (int w : c->model->stat_widths()) { x.sync_off.push_back(off); off += 4 * (int64_t)w; }
    int rc = dev_alloc(&x.sync_buf, (size_t)off);
    if (rc) return rc;
  }
  return MWW_OK;
}

int mww_allreduce_unique_id(void* out_id, int capacity) {
  if (!out_id || capacity < MWW_UNIQUE_ID_BYTES) return fail(MWW_ERR_INVALID, "unique-id buffer too small");
  static RcclApi api;
  int rc = rccl_load(&api);
  if (rc) return rc;
  RcclApi::UniqueId id;
  const int e = api.GetUniqueId(&id);
  if (e != 0) return fail(MWW_ERR_HIP, std::string("ncclGetUniqueId: ") + api.GetErrorString(e));
  memcpy(out_id, id.internal, sizeof(id.internal));
  return MWW_OK;
}

int mww_allreduce_destroy(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  RcclState* r = c->xch.rccl;
  if (!r) return MWW_OK;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (r->side) (void)hipStreamSynchronize(r->side);
  if (c->xch.hook == rccl_exchange) {
    c->xch.hook = nullptr;
    c->xch.user = nullptr;
    c->xch.world = 1;
    c->xch.sync_bn = c->xch.reduce_grads = false;
  }
  if (r->comm) (void)r->api.CommDestroy(r->comm);
  if (r->side) (void)hipStreamDestroy(r->side);
  if (r->ev_ready) (void)hipEventDestroy(r->ev_ready);
  if (r->ev_done) (void)hipEventDestroy(r->ev_done);
  delete r;
  c->xch.rccl = nullptr;
  return MWW_OK;
}

int mww_allreduce_world(mww_ctx* c) {
  if (!c) return fail(MWW_ERR_INVALID, "null context");
  RcclState* r = c->xch.rccl;
  if (!r || !r->comm) return 0;
  int n = 0;
  if (!r->api.CommCount) return fail(MWW_ERR_UNSUPPORTED, "librccl.so lacks ncclCommCount");
  const int e = r->api.CommCount(r->comm, &n);
  if (e != 0) return fail(MWW_ERR_HIP, std::string("ncclCommCount: ") + r->api.GetErrorString(e));
  return n;
}

int mww_allreduce_init(mww_ctx* c, int rank, int world, const void* unique_id, int sync_bn) {
  if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return fail(MWW_ERR_INVALID, "bad rank / world size");
  MWW_TRY(single_device_only(c, nullptr));   // (before the communicator is touched: a refused call leaves the context as it was)
  int rc = mww_allreduce_destroy(c);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  RcclState* r = new RcclState();
  r->c = c;
  rc = rccl_load(&r->api);
  if (rc) { delete r; return rc; }
  RcclApi::UniqueId id;
  memcpy(id.internal, unique_id, sizeof(id.internal));
  const int e = r->api.CommInitRank(&r->comm, world, id, rank);
  if (e != 0) {
    const std::string msg = std::string("ncclCommInitRank: ") + r->api.GetErrorString(e);
    delete r;
    return fail(MWW_ERR_HIP, msg);
  }
  c->xch.rccl = r;
  HIPCHK(hipStreamCreateWithFlags(&r->side, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&r->ev_ready, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&r->ev_done, hipEventDisableTiming));
  return mww_set_allreduce_hook(c, rccl_exchange, r, world, sync_bn, 1);
}

}  // extern "C"
