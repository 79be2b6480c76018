// Flash attention kernels instantiated for head dim 256 (launchers: attention_impl.h; kernels: attention_fwd.h, attention_bwd.h).
#include "attention_impl.h"

namespace apex {

int attn_fwd_d256(const AttnArgs& a, int dt, hipStream_t s) { return attn_fwd_impl<256>(a, dt, s); }

int attn_bwd_d256(const AttnArgs& a, const void* dout, float* delta_ws, void* dk, void* dv, int dt, hipStream_t s) {
  return attn_bwd_impl<256>(a, dout, delta_ws, dk, dv, dt, s);
}

}  // namespace apex
