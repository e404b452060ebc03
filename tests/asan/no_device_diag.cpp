// TEST INFRASTRUCTURE ONLY — the sanitizer build of the host code (see no_device.cpp): ke_diagnose's device entry
// point answered "no device".  The product library never links this file.
#include "../../koordinator_amd/csrc/ke_host.h"

namespace ke {
int device_diagnose(Context*, int32_t, const ke_pod*, int64_t, ke_pod_diagnosis*, int32_t, uint64_t* const*) {
  return fail(KE_ERR_NO_DEVICE, "sanitizer build: no device");
}
}  // namespace ke
