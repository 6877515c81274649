// Host glue of the entry points that take host pointers or chain fallible steps (witness.hip, resident.hip, layout.hip): an owned
// device buffer, the early return on a failed step, uploads and downloads on the context's stream, the kernels' error word.
#pragma once
#include "common.hpp"

namespace vdb {

// ------------------------------------------------------------------ helpers for the host-pointer ABI
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  int alloc(size_t bytes) {
    hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc", __FILE__, __LINE__);
    return VDB_OK;
  }
  template <class U>
  U* as() { return (U*)p; }
};
#define TRY(x)             \
  do {                     \
    int _rc = (x);         \
    if (_rc) return _rc;   \
  } while (0)

static int check_err_flag(int* derr) {
  int h = 0;
  VDB_HIP(hipMemcpyAsync(&h, derr, sizeof(int), hipMemcpyDeviceToHost, ctx().stream));
  VDB_HIP(hipStreamSynchronize(ctx().stream));
  if (h) {
    set_error("data-dependent failure the reference turns into a panic (division by zero / index out of range)");
    return VDB_ERR_DOMAIN;
  }
  return VDB_OK;
}

// upload helper for the host-pointer entry points
static int upload(DevBuf& d, const void* src, size_t bytes) {
  TRY(d.alloc(bytes));
  if (bytes) VDB_HIP(hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, ctx().stream));
  return VDB_OK;
}
static int download(void* dst, const void* src, size_t bytes) {
  if (dst && bytes) VDB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx().stream));
  return VDB_OK;
}

}  // namespace vdb
