// The single exchange of a training step for callers that do not bring torch.distributed: one
// in-place sum over ranks of the packed [loss_sum | grad_sum | sample count] buffer with RCCL over xGMI
// (the jnp.mean at reference policy/base.py:126-127 and gan/js_policy.py:55).
//
// RCCL is bound at run time (dlopen + dlsym) instead of at link time: inside a PyTorch process the
// library torch already loaded is the one found (one RCCL, one HIP runtime per process); a plain C
// caller gets /opt/rocm's.  A ctx that never called gmpc_comm_init is a world of one and the exchange
// is a no-op, so single-GPU callers need no RCCL at all.
#include <dlfcn.h>
#include <cstdio>
#include <cstring>

#include "gmpc_launch.h"

namespace {
struct NcclId { char internal[128]; };           // ncclUniqueId (NCCL_UNIQUE_ID_BYTES = 128)
typedef void* NcclComm;
typedef int (*fn_get_id)(NcclId*);
typedef int (*fn_init_rank)(NcclComm*, int, NcclId, int);
typedef int (*fn_allreduce)(const void*, void*, size_t, int, int, NcclComm, hipStream_t);
typedef int (*fn_destroy)(NcclComm);
typedef const char* (*fn_errstr)(int);
enum { kNcclFloat32 = 7, kNcclSum = 0 };         // ncclDataType_t / ncclRedOp_t values of rccl.h

struct Rccl {
  void* handle = nullptr;
  fn_get_id get_id = nullptr;
  fn_init_rank init_rank = nullptr;
  fn_allreduce allreduce = nullptr;
  fn_destroy destroy = nullptr;
  fn_errstr errstr = nullptr;
  char why[256] = "";
};

Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (tried) return &r;
  tried = true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* nm : names) {
    r.handle = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
    if (r.handle) break;
  }
  if (!r.handle) {
    snprintf(r.why, sizeof(r.why), "librccl.so not found: %s", dlerror());
    return &r;
  }
  r.get_id = reinterpret_cast<fn_get_id>(dlsym(r.handle, "ncclGetUniqueId"));
  r.init_rank = reinterpret_cast<fn_init_rank>(dlsym(r.handle, "ncclCommInitRank"));
  r.allreduce = reinterpret_cast<fn_allreduce>(dlsym(r.handle, "ncclAllReduce"));
  r.destroy = reinterpret_cast<fn_destroy>(dlsym(r.handle, "ncclCommDestroy"));
  r.errstr = reinterpret_cast<fn_errstr>(dlsym(r.handle, "ncclGetErrorString"));
  if (!r.get_id || !r.init_rank || !r.allreduce || !r.destroy) {
    snprintf(r.why, sizeof(r.why), "librccl.so lacks one of ncclGetUniqueId / ncclCommInitRank / "
                                   "ncclAllReduce / ncclCommDestroy");
    r.handle = nullptr;
  }
  return &r;
}
}  // namespace

int gmpc_comm_unique_id_impl(char* id128) {
  Rccl* r = rccl();
  if (!r->handle) return gmpc_fail(GMPC_EINVAL, "RCCL unavailable: %s", r->why);
  NcclId id;
  const int rc = r->get_id(&id);
  if (rc != 0) return gmpc_fail(GMPC_EHIP, "ncclGetUniqueId failed: %s", r->errstr ? r->errstr(rc) : "?");
  memcpy(id128, id.internal, sizeof(id.internal));
  return 0;
}

int gmpc_comm_init_impl(GmpcComm* gc, int world, int rank, const char* id128) {
  if (world < 1 || rank < 0 || rank >= world) return gmpc_fail(GMPC_EINVAL, "rank %d of %d", rank, world);
  Rccl* r = rccl();
  if (!r->handle) return gmpc_fail(GMPC_EINVAL, "RCCL unavailable: %s", r->why);
  if (gc->comm) { r->destroy(gc->comm); gc->comm = nullptr; }
  NcclId id;
  memcpy(id.internal, id128, sizeof(id.internal));
  const int rc = r->init_rank(&gc->comm, world, id, rank);
  if (rc != 0) {
    gc->comm = nullptr;
    return gmpc_fail(GMPC_EHIP, "ncclCommInitRank(%d of %d) failed: %s", rank, world,
                     r->errstr ? r->errstr(rc) : "?");
  }
  gc->world = world;
  gc->rank = rank;
  return 0;
}

int gmpc_comm_allreduce_impl(GmpcComm* gc, float* packed, long count, hipStream_t s) {
  if (!gc->comm) return 0;                       // a world of one: nothing to exchange
  Rccl* r = rccl();
  const int rc = r->allreduce(packed, packed, (size_t)count, kNcclFloat32, kNcclSum, gc->comm, s);
  if (rc != 0) return gmpc_fail(GMPC_EHIP, "ncclAllReduce failed: %s", r->errstr ? r->errstr(rc) : "?");
  return 0;
}

void gmpc_comm_destroy_impl(GmpcComm* gc) {
  if (gc->comm) {
    Rccl* r = rccl();
    if (r->handle) r->destroy(gc->comm);
    gc->comm = nullptr;
  }
  gc->world = 1;
  gc->rank = 0;
}
