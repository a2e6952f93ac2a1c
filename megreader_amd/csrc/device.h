// Host-side state the library keeps per device (defined in elementwise.hip): every table is indexed by current_device() and holds
// MR_MAX_DEVICES entries; a device index beyond that is refused, never wrapped.
#pragma once
#include "common.h"

namespace mr {

int current_device();   // the calling thread's current device; -1 when there is none or its index is >= MR_MAX_DEVICES

// Compute units of the current device (cached per device); 0 when there is none.  What "no device" means is the caller's choice:
// mr_decode_persist_ok answers "does not fit" (device_cus), the NT / TN planners assume the whole MI355X (num_cus), so that their
// host-only queries (mr_nt_kernel_code, ...) answer the same with and without a GPU.
int device_cus();
inline int num_cus() {
  const int n = device_cus();
  return n > 0 ? n : 256;
}

// One 4 KiB page of zeros per device: the source of padded vectors for the direct-to-LDS loads.  Created on first use (mr_init()
// creates it eagerly, e.g. before hipGraph capture); null when it cannot be.
const void* zero_page();

// Raises the kernel's dynamic-LDS limit to `bytes` once per (kernel, device).  MR_OK, or MR_ERR_LAUNCH with the error set.
int ensure_dynamic_lds(const void* kernel, size_t bytes);
template <typename... A>
inline int ensure_dynamic_lds(void (*kernel)(A...), size_t bytes) { return ensure_dynamic_lds((const void*)kernel, bytes); }

}  // namespace mr
