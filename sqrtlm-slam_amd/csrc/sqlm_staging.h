// sqlm_staging.h — host code shared by the batched solvers (sqlm_sim3.cpp,
// sqlm_pose.cpp, sqlm_lidar.cpp): every call lays its arrays out in a few
// arenas, uploads the input arena from a pinned mirror in one copy and reads
// the output arena back the same way. The buffers belong to the solver, grow on
// demand and are reused by the next call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/sqrtlm.h"

namespace sqlm {

// A device buffer and (with_host) a pinned host mirror of the same size.
struct Staged {
  char *dev = nullptr, *host = nullptr;
  size_t cap = 0;

  Staged() = default;
  Staged(const Staged &) = delete;
  Staged &operator=(const Staged &) = delete;
  ~Staged() { release(); }

  // At least `need` bytes; the contents do not survive a growth. On failure
  // the object is left empty.
  int grow(size_t need, bool with_host = true) {
    if (need <= cap) return SQLM_OK;
    release();
    const size_t n = need + need / 2;
    if (hipMalloc((void **)&dev, n) != hipSuccess ||
        (with_host && hipHostMalloc((void **)&host, n, hipHostMallocDefault) != hipSuccess)) {
      release();
      return SQLM_ERR_OOM;
    }
    cap = n;
    return SQLM_OK;
  }

 private:
  void release() {
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    dev = host = nullptr;
    cap = 0;
  }
};

// bump allocation in 16-byte steps
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += (bytes + 15) & ~(size_t)15;
    return o;
  }
};

// the array an Arena placed at `off` of a buffer
template <class T>
T *at(char *base, size_t off) {
  return reinterpret_cast<T *>(base + off);
}

}  // namespace sqlm
