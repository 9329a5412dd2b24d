// Host-side helpers of the HIP translation units (sem_internal.h is also built by the host compiler alone).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <type_traits>

#include "sem_internal.h"

namespace sem {

inline int hip_check(hipError_t e, const char* what) {
  if (e == hipSuccess) return SEM_OK;
  return set_error(SEM_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Calls f(std::integral_constant<int, P>) for the compiled order P == order (1..kMaxOrder) and returns its status.
template <int P = 1, class F>
int dispatch_order(int order, F&& f) {
  if constexpr (P > kMaxOrder) {
    return set_error(SEM_EUNSUPPORTED, "polynomial order outside compiled range");
  } else {
    if (order == P) return f(std::integral_constant<int, P>{});
    return dispatch_order<P + 1>(order, f);
  }
}

}  // namespace sem
