// mom_comm.hip -- the multi-GPU part of the C ABI (include/momcore.h): RCCL, loaded on first use, behind mom_comm_* and
// mom_allgather*.  Plain host code: no kernel is launched from here.
#include <cstring>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: the library itself is dlopen'ed by mom_comm_init

#include "mom_handle.hpp"

void (*g_rccl_destroy)(void *) = nullptr;  // set once RCCL is loaded (mom_comm_init)

namespace {
struct Rccl {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
Rccl g_rccl;
// librccl.so.1 is loaded on first use (the soname a host process such as PyTorch-ROCm may already have mapped: one
// copy per process); libmomcore.so itself stays loadable on machines without RCCL
int rccl_load(mom_t *h) {
  if (g_rccl.lib) return MOM_OK;
  // RCCL must sit on the SAME HIP runtime instance as this library.  A host process may hold two (PyTorch-ROCm wheels
  // bundle libamdhip64.so + librccl.so next to /opt/rocm's, and which one libmomcore.so was bound to depends on the
  // import order), so the copy next to the runtime that resolves OUR hip* symbols is taken first
  void *lib = nullptr;
  Dl_info info;
  if (dladdr(reinterpret_cast<void *>(&hipGetDeviceCount), &info) && info.dli_fname) {
    std::string dir(info.dli_fname);
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos) {
      dir.resize(slash);
      for (const char *name : {"/librccl.so.1", "/librccl.so"}) {
        lib = dlopen((dir + name).c_str(), RTLD_NOW | RTLD_LOCAL);
        if (lib) break;
      }
    }
  }
  if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
  if (!lib) return fail(h, MOM_EHIP, "mom_comm: cannot load librccl.so.1 (RCCL)");
  Rccl r;
  r.lib = lib;
  *(void **)(&r.GetUniqueId) = dlsym(lib, "ncclGetUniqueId");
  *(void **)(&r.CommInitRank) = dlsym(lib, "ncclCommInitRank");
  *(void **)(&r.CommDestroy) = dlsym(lib, "ncclCommDestroy");
  *(void **)(&r.AllGather) = dlsym(lib, "ncclAllGather");
  *(void **)(&r.AllReduce) = dlsym(lib, "ncclAllReduce");
  *(void **)(&r.GetErrorString) = dlsym(lib, "ncclGetErrorString");
  if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather || !r.AllReduce || !r.GetErrorString)
    return fail(h, MOM_EHIP, "mom_comm: librccl.so.1 lacks a required symbol");
  g_rccl = r;
  g_rccl_destroy = [](void *c) { (void)g_rccl.CommDestroy((ncclComm_t)c); };
  return MOM_OK;
}
int rccl_fail(mom_t *h, const char *what, ncclResult_t r) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s failed: %s", what, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  return fail(h, MOM_EHIP, buf);
}
}  // namespace

extern "C" int mom_comm_unique_id(void *id_out, size_t bytes) {
  if (!id_out || bytes < sizeof(ncclUniqueId)) return fail(nullptr, MOM_EINVAL, "mom_comm_unique_id: need MOM_COMM_ID_BYTES bytes");
  const int rc = rccl_load(nullptr);
  if (rc) return rc;
  ncclUniqueId id;
  const ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) return rccl_fail(nullptr, "ncclGetUniqueId", r);
  memcpy(id_out, &id, sizeof id);
  return MOM_OK;
}

extern "C" int mom_comm_init(mom_t *h, int rank, int nranks, const void *nccl_id) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (nranks < 1 || rank < 0 || rank >= nranks || !nccl_id) return fail(h, MOM_EINVAL, "mom_comm_init: bad argument");
  if (h->comm) return fail(h, MOM_ESTATE, "mom_comm_init: communicator already initialised");
  HIPCHK(h, hipSetDevice(h->device));
  const int rc = rccl_load(h);
  if (rc) return rc;
  // RCCL checks hipGetLastError() after its own launches: a stale (non-sticky) error code left behind by an earlier,
  // already reported failure in this process would be taken for its own
  (void)hipGetLastError();
  ncclUniqueId id;
  memcpy(&id, nccl_id, sizeof id);
  ncclComm_t comm = nullptr;
  const ncclResult_t r = g_rccl.CommInitRank(&comm, nranks, id, rank);
  if (r != ncclSuccess) return rccl_fail(h, "ncclCommInitRank", r);
  h->comm = comm; h->comm_rank = rank; h->comm_size = nranks;
  return MOM_OK;
}

extern "C" int mom_comm_destroy(mom_t *h) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (h->comm) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)g_rccl.CommDestroy((ncclComm_t)h->comm);
    h->comm = nullptr; h->comm_size = 1; h->comm_rank = 0;
  }
  return MOM_OK;
}

// get_dtau_ndoubl's maximum over the whole spectral axis (mom_scene_set_optics): the per-layer maxima of the ranks, in place
int mom_comm_allreduce_max(mom_t *h, double *d_buf, size_t count) {
  const ncclResult_t r = g_rccl.AllReduce(d_buf, d_buf, count, ncclDouble, ncclMax, (ncclComm_t)h->comm, h->stream);
  if (r != ncclSuccess) return rccl_fail(h, "ncclAllReduce", r);
  return MOM_OK;
}

extern "C" int mom_allgather(mom_t *h, const void *d_local, void *d_global, size_t count) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  if (!h->comm) return fail(h, MOM_ESTATE, "mom_allgather: call mom_comm_init first");
  if (!d_local || !d_global) return fail(h, MOM_EINVAL, "mom_allgather: null buffer");
  HIPCHK(h, hipSetDevice(h->device));
  const ncclResult_t r = g_rccl.AllGather(d_local, d_global, count, ncclDouble, (ncclComm_t)h->comm, h->stream);
  if (r != ncclSuccess) return rccl_fail(h, "ncclAllGather", r);
  return MOM_OK;
}

// The ONE collective of a sharded run: every rank contributes its R_SFI || T_SFI block (already contiguous in the
// handle, 2 * nVza * nStokes * S_loc doubles) and receives [nranks][2][nVza*nStokes*S_loc]
extern "C" int mom_allgather_RT_device(mom_t *h, void *d_global) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_allgather_RT_device");
  if (!h->scene_set || !d_global) return fail(h, MOM_ESTATE, "mom_allgather_RT_device: no scene / null output");
  return mom_allgather(h, h->d_R, d_global, 2 * (size_t)h->nVza * h->nS * h->S);
}

extern "C" int mom_allgather_RT(mom_t *h, double *R_SFI_global, double *T_SFI_global) {
  if (!h) return fail(nullptr, MOM_EINVAL, "null handle");
  F64_ONLY(h, "mom_allgather_RT");
  if (!h->scene_set || !R_SFI_global || !T_SFI_global) return fail(h, MOM_ESTATE, "mom_allgather_RT: no scene / null output");
  if (!h->comm) return fail(h, MOM_ESTATE, "mom_allgather_RT: call mom_comm_init first");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t nout = (size_t)h->nVza * h->nS * h->S, need = 2 * nout * h->comm_size;
  HIPCHK(h, h->d_gather.reserve(need, h->stream));
  int rc = mom_allgather_RT_device(h, h->d_gather);
  if (rc) return rc;
  // [rank][R|T][nVza, nStokes, S_loc] -> R_SFI, T_SFI [nVza, nStokes, nranks * S_loc] (rank-major spectral axis)
  for (int r = 0; r < h->comm_size; ++r) {
    HIPCHK(h, hipMemcpyAsync(R_SFI_global + nout * r, h->d_gather + 2 * nout * r, nout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(T_SFI_global + nout * r, h->d_gather + 2 * nout * r + nout, nout * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  return check_info(h);
}
