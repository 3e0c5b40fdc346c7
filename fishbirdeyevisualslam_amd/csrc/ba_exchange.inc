// ba_exchange.inc -- exchange transport of the landmark-sharded BA (included by ba.hip).
//
// RCCL: the all-reduces are enqueued on the BA's stream and work on device buffers (nothing is staged through the host);
// the entry points are resolved at run time from the RCCL the process already has (torch's librccl.so.1 when the host is
// Python, /opt/rocm/lib otherwise), so the library carries no link-time dependency and single-GPU users never load it.
// HOST: the fb_allreduce_fn callback of fb_local_ba_sharded (gloo in the CPU tests; host buffer).
#include <dlfcn.h>
namespace {
struct RcclApi {
  void *lib = nullptr;
  int (*GetUniqueId)(void *) = nullptr;                              // ncclGetUniqueId(ncclUniqueId *)
  int (*CommInitRank)(void **, int, fb_rccl_unique_id, int) = nullptr; // ncclCommInitRank(comm *, nranks, id BY VALUE, rank)
  int (*CommDestroy)(void *) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
  int (*CommCount)(void *, int *) = nullptr;
  int (*CommUserRank)(void *, int *) = nullptr;
};
RcclApi *rccl_api() {
  // loaded once (a function-local static is initialised thread-safely)
  static RcclApi api = [] {
    RcclApi a;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      a.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (a.lib) break;
    }
    if (a.lib) {
      a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(a.lib, "ncclGetUniqueId"));
      a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(a.lib, "ncclCommInitRank"));
      a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
      a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(dlsym(a.lib, "ncclAllReduce"));
      a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
      a.CommCount = reinterpret_cast<decltype(a.CommCount)>(dlsym(a.lib, "ncclCommCount"));
      a.CommUserRank = reinterpret_cast<decltype(a.CommUserRank)>(dlsym(a.lib, "ncclCommUserRank"));
      if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllReduce) a.lib = nullptr;
    }
    return a;
  }();
  return api.lib ? &api : nullptr;
}
constexpr int kNcclDouble = 8, kNcclSum = 0;  // ncclFloat64, ncclSum (rccl.h)

struct Xchg {
  int world = 1;
  void *comm = nullptr;            // ncclComm_t, or
  fb_allreduce_fn cb = nullptr;    // host callback
  void *ctx = nullptr;
  bool active() const { return world > 1 || comm != nullptr; }  // a 1-rank communicator still goes through RCCL (tests)
  // in-place sum over the ranks of n doubles in DEVICE memory, ordered behind the work already on stream s
  // (src may differ from dbuf: out-of-place, the source stays as it is)
  int sum_dev(double *dbuf, size_t n, hipStream_t s, std::vector<double> &scratch, const double *src = nullptr) const {
    if (!src) src = dbuf;
    if (!active() || n == 0) return FB_OK;
    if (comm) {
      const int rc = rccl_api()->AllReduce(src, dbuf, n, kNcclDouble, kNcclSum, comm, s);
      if (rc != 0) { fb::set_error("fb_local_ba_sharded: ncclAllReduce failed: %s", rccl_api()->GetErrorString ? rccl_api()->GetErrorString(rc) : "?"); return FB_ERR_HIP; }
      return FB_OK;
    }
    scratch.resize(n);
    FB_HIP(hipStreamSynchronize(s));
    FB_HIP(hipMemcpy(scratch.data(), src, n * 8, hipMemcpyDeviceToHost));
    if (cb(ctx, scratch.data(), (int32_t)n, 0) != 0) { fb::set_error("fb_local_ba_sharded: all-reduce callback failed"); return FB_ERR_ARG; }
    FB_HIP(hipMemcpy(dbuf, scratch.data(), n * 8, hipMemcpyHostToDevice));
    return FB_OK;
  }
  // in-place reduction of n doubles in HOST memory (op 0 = sum, 1 = max): the argument agreement before anything is enqueued
  int reduce_host(double *hbuf, int n, int op) const {
    if (!active() || n <= 0) return FB_OK;
    if (cb) {
      if (cb(ctx, hbuf, n, op) != 0) { fb::set_error("fb_local_ba_sharded: all-reduce callback failed"); return FB_ERR_ARG; }
      return FB_OK;
    }
    fb::DevBuf d;
    FB_TRY(d.upload(hbuf, (size_t)n * 8));
    const int rc = rccl_api()->AllReduce(d.p, d.p, (size_t)n, kNcclDouble, op == 0 ? kNcclSum : 2 /* ncclMax */, comm, nullptr);
    if (rc != 0) { fb::set_error("fb_local_ba_sharded: ncclAllReduce failed (%d)", rc); return FB_ERR_HIP; }
    FB_HIP(hipStreamSynchronize(nullptr));
    return d.download(hbuf, (size_t)n * 8);
  }
};
}  // namespace

extern "C" int fb_rccl_get_unique_id(fb_rccl_unique_id *id) {
  FB_ARG(id);
  RcclApi *r = rccl_api();
  if (!r) { fb::set_error("fb_rccl_get_unique_id: no RCCL in this process (librccl.so.1 not found)"); return FB_ERR_NODEVICE; }
  const int rc = r->GetUniqueId(id);
  if (rc != 0) { fb::set_error("ncclGetUniqueId failed (%d)", rc); return FB_ERR_HIP; }
  return FB_OK;
}
extern "C" int fb_rccl_comm_info(void *comm, int *count, int *rank) {
  FB_ARG(comm && count && rank);
  RcclApi *r = rccl_api();
  if (!r || !r->CommCount || !r->CommUserRank) { fb::set_error("fb_rccl_comm_info: ncclCommCount / ncclCommUserRank not available"); return FB_ERR_NODEVICE; }
  int rc = r->CommCount(comm, count);
  if (rc == 0) rc = r->CommUserRank(comm, rank);
  if (rc != 0) { fb::set_error("fb_rccl_comm_info: RCCL error %d", rc); return FB_ERR_HIP; }
  return FB_OK;
}
extern "C" int fb_rccl_comm_init(const fb_rccl_unique_id *id, int rank, int world, void **comm) {
  FB_TRY(fb::check_device());
  FB_ARG(id && comm && world >= 1 && rank >= 0 && rank < world);
  RcclApi *r = rccl_api();
  if (!r) { fb::set_error("fb_rccl_comm_init: no RCCL in this process (librccl.so.1 not found)"); return FB_ERR_NODEVICE; }
  const int rc = r->CommInitRank(comm, world, *id, rank);
  if (rc != 0) { fb::set_error("ncclCommInitRank failed: %s", r->GetErrorString ? r->GetErrorString(rc) : "?"); return FB_ERR_HIP; }
  return FB_OK;
}
extern "C" int fb_rccl_comm_destroy(void *comm) {
  RcclApi *r = rccl_api();
  if (comm && r) r->CommDestroy(comm);
  return FB_OK;
}
