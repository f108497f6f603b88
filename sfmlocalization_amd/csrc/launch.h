// Launches: every kernel of the library is launched by dev_launch below -- directly, or through sfm_launch<Body>
// (sfmloc_internal.h) and the gang launches of gang.h, which end here too.  One call converts the arguments, raises the
// kernel's dynamic-LDS limit where the launch needs it (devmem.h "Dynamic-LDS limits": the rule, and what is not known
// about it), launches, and checks: one check per launch, with the launch site in the error text.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "devmem.h"

namespace sfmloc {

// the SFMLOC code of a failed HIP call
inline int hip_code(hipError_t e) {
  return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? SFMLOC_ENODEV
         : (e == hipErrorOutOfMemory)                          ? SFMLOC_ENOMEM
                                                               : SFMLOC_EHIP;
}

// Where a launch is written: what a call's first converted argument (the stream of dev_launch, the member of sfm_launch)
// carries along, its defaults being evaluated at the call.  The rule for a wrapper around dev_launch: it declares its
// stream parameter as a LaunchStream (gp_launch, ws_launch) and passes it on, so the site is its caller's; a wrapper
// that takes a hipStream_t and forwards it would report its own line for every launch, without any warning.
struct LaunchSite {
  const char *file;
  int line;
};
// the stream to launch on -- anything that reads as a hipStream_t -- and the site; `device`: the ordinal of the device
// that is current where the caller knows it (a gang member's), else -1 and dev_launch asks the runtime when it needs it
struct LaunchStream {
  hipStream_t s;
  LaunchSite at;
  int device = -1;
  template <class S, class = std::enable_if_t<std::is_convertible_v<S, hipStream_t>>>
  LaunchStream(S &&s_, const char *file = __builtin_FILE(), int line = __builtin_LINE())
      : s(static_cast<hipStream_t>(s_)), at{file, line} {}
  LaunchStream(hipStream_t s_, LaunchSite at_, int device_) : s(s_), at(at_), device(device_) {}
};

// kernel<<<grid, block, lds_bytes, stream>>>(args...), each argument converted to the kernel's own parameter type (a
// DevBuf<T> or a T * for a const T *, a size_t for a uint32_t).  SFMLOC_OK, or the launch's code with the error text set.
template <class... Ts, class... As>
inline int dev_launch(void (*kernel)(Ts...), dim3 grid, dim3 block, size_t lds_bytes, LaunchStream on, As &&...as) {
  static_assert(sizeof...(Ts) == sizeof...(As), "one argument for each of the kernel's parameters");
  if (lds_bytes > kLdsDefaultLimit) {
    int device = on.device;  // (left at -1 by a failed call: no mark, the limit is raised for this launch alone)
    if (device < 0) (void)hipGetDevice(&device);
    const int rc = lds_allow(reinterpret_cast<const void *>(kernel), device, (uint32_t)lds_bytes);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(kernel, grid, block, (uint32_t)lds_bytes, on.s, static_cast<Ts>(as)...);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return SFMLOC_OK;
  set_error("%s:%d launch (grid %u x %u x %u, %u threads, %zu B LDS) -> %s", on.at.file, on.at.line, grid.x, grid.y,
            grid.z, block.x * block.y * block.z, lds_bytes, hipGetErrorString(e));
  return hip_code(e);
}

}  // namespace sfmloc
