// art_rccl.cpp -- the radiated-flux reduction across ranks: one RCCL all-reduce
// (art_comm_*, art_flux_allreduce*, declared in include/art.h).
// RCCL is opened at first use (dlopen), so libart.so loads and runs single-GPU work where it
// is absent; a process that already loaded librccl.so.1 (e.g. PyTorch's) shares that copy.
#include <dlfcn.h>

#include "art_host.h"

using namespace art::host;

namespace {
typedef int (*nccl_get_id_t)(void*);
typedef int (*nccl_init_rank_t)(void**, int, art_rccl_id, int);
typedef int (*nccl_allreduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_destroy_t)(void*);
typedef const char* (*nccl_err_t)(int);
struct Rccl {
  void* h = nullptr;
  nccl_get_id_t get_id = nullptr;
  nccl_init_rank_t init_rank = nullptr;
  nccl_allreduce_t allreduce = nullptr;
  nccl_destroy_t destroy = nullptr;
  nccl_err_t err = nullptr;
  void* comm = nullptr;
  int device = -1;
};
Rccl g_rccl;
constexpr int NCCL_FLOAT64 = 8;  // ncclFloat64 (rccl.h)
constexpr int NCCL_SUM = 0;      // ncclSum

int rccl_open() {
  if (g_rccl.h) return ART_OK;
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return fail(ART_E_UNSUPPORTED, "RCCL (librccl.so.1) is not available: %s", dlerror());
  g_rccl.get_id = (nccl_get_id_t)dlsym(h, "ncclGetUniqueId");
  g_rccl.init_rank = (nccl_init_rank_t)dlsym(h, "ncclCommInitRank");
  g_rccl.allreduce = (nccl_allreduce_t)dlsym(h, "ncclAllReduce");
  g_rccl.destroy = (nccl_destroy_t)dlsym(h, "ncclCommDestroy");
  g_rccl.err = (nccl_err_t)dlsym(h, "ncclGetErrorString");
  if (!g_rccl.get_id || !g_rccl.init_rank || !g_rccl.allreduce || !g_rccl.destroy || !g_rccl.err)
    return fail(ART_E_UNSUPPORTED, "librccl.so.1 lacks the nccl* entry points");
  g_rccl.h = h;
  return ART_OK;
}

int rccl_fail(int r, const char* what) {
  return fail(ART_E_HIP, "%s: %s", what, g_rccl.err ? g_rccl.err(r) : "RCCL error");
}
}  // namespace

extern "C" {

int art_comm_unique_id(art_rccl_id* id) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!id) return fail(ART_E_INVALID, "id is NULL");
  int rc = rccl_open();
  if (rc) return rc;
  const int r = g_rccl.get_id(id);
  return r ? rccl_fail(r, "ncclGetUniqueId") : ART_OK;
}

int art_comm_init(int32_t rank, int32_t world, const art_rccl_id* id) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!id || world < 1 || rank < 0 || rank >= world) return fail(ART_E_INVALID, "bad rank/world/id");
  if (g_rccl.comm) return fail(ART_E_INVALID, "communicator already initialised (art_comm_destroy first)");
  int rc = rccl_open();
  if (rc) return rc;
  int dev = 0;
  HIP_OK(hipGetDevice(&dev));
  void* comm = nullptr;
  const int r = g_rccl.init_rank(&comm, world, *id, rank);
  if (r) return rccl_fail(r, "ncclCommInitRank");
  g_rccl.comm = comm;
  g_rccl.device = dev;
  return ART_OK;
}

int art_flux_allreduce(double* buf, int64_t count, void* stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_rccl.comm) return fail(ART_E_INVALID, "no communicator: art_comm_init first");
  if (count < 0 || (count > 0 && !buf)) return fail(ART_E_INVALID, "bad buffer");
  if (count == 0) return ART_OK;
  const int r = g_rccl.allreduce(buf, buf, (size_t)count, NCCL_FLOAT64, NCCL_SUM, g_rccl.comm, (hipStream_t)stream);
  return r ? rccl_fail(r, "ncclAllReduce") : ART_OK;
}

// The same for a host buffer (a Julia host's Vector{Float64}): staged through HBM on the
// library's stream, reduced, copied back; synchronous.
int art_flux_allreduce_host(double* buf, int64_t count) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_rccl.comm) return fail(ART_E_INVALID, "no communicator: art_comm_init first");
  if (count < 0 || (count > 0 && !buf)) return fail(ART_E_INVALID, "bad buffer");
  if (count == 0) return ART_OK;
  DeviceCtx* c;
  int rc = current_ctx(&c);
  if (rc) return rc;
  void* d;
  if ((rc = pool_get(c, 8, (size_t)count * sizeof(double), &d))) return rc;
  HIP_OK(hipMemcpyAsync(d, buf, (size_t)count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const int r = g_rccl.allreduce(d, d, (size_t)count, NCCL_FLOAT64, NCCL_SUM, g_rccl.comm, c->stream);
  if (r) return rccl_fail(r, "ncclAllReduce");
  HIP_OK(hipMemcpyAsync(buf, d, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return ART_OK;
}

int art_comm_destroy(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_rccl.comm) return ART_OK;
  const int r = g_rccl.destroy(g_rccl.comm);
  g_rccl.comm = nullptr;
  return r ? rccl_fail(r, "ncclCommDestroy") : ART_OK;
}

}  // extern "C"
