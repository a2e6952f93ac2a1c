// The granule exchange of the persistent kernels (lstm_persist.hip: 4 workgroups per batch group; decode_persist.hip: 32): how the
// workgroups of ONE launch hand data to each other, and the workspace those hand-offs live in.
//
// Inter-workgroup protocol (MI355X_MICROARCH.md "Workgroup dispatch, XCD placement & inter-workgroup visibility",
// cdna_hip_programming.md Guideline 16 form R2): granule = one naturally aligned 8-byte {value, tag} written by ONE store
// (global_store_dwordx2/x4 sc1, or plain once the group is known to share an XCD: gran2_publish) and read by relaxed agent-scope
// loads (sc1, L1-bypassing): the data is its own flag -- no fence, no separate flag round trip; placement-independent, no
// dependence on dispatch order beyond co-residency of the members of a group.  tag = step + 1 (never 0); the exchange buffer is
// zero at every launch (a memset node ahead of it, or a caller that zeroed it: persist_ws_prepare); two slots alternate (a
// producer can run at most one step ahead of its slowest consumer).  Every spin is bounded: on timeout the workgroup records a
// code in the status block, stops waiting (no hang) and POISONS its outputs with NaN, so the failure reaches the loss / the
// gradients instead of silently corrupting a training run.
//
// Workspace: [granule slots][XCC-id exchange ("hello")][status block, PERSIST_STATUS_BYTES].
#pragma once
#include "common.h"
#include "igemm_core.h"   // rsrc_t, make_rsrc

namespace mr {

typedef unsigned long long u64;
constexpr int AUX_SC1 = 16;   // cache-policy bit of the raw buffer builtins: sc1 = agent scope (write-through / L1 bypass)
constexpr unsigned SPIN_LIMIT = 1u << 21;
constexpr unsigned HELLO_TAG = 0x48454C4Fu;
constexpr unsigned TIMING_MAGIC = 0x54494D45u;

// the status block: the last bytes of the workspace, as 32-bit words
constexpr int PERSIST_STATUS_BYTES = 256;
constexpr int PERSIST_ST_TIMEOUT = 0;     // code of the hand-off that timed out (atomicMax), 0 = none
constexpr int PERSIST_ST_COLOCATED = 1;   // workgroups that found their batch group on one XCD
constexpr int PERSIST_ST_TIMING = 2;      // the CALLER sets TIMING_MAGIC here to switch the phase clocks on (tools/ only)
constexpr int PERSIST_ST_TICKS = 8;       // first word of the phase clocks

// Two adjacent granules travel as ONE 16-byte sc1 access: {value0, tag, value1, tag}.  Each 8-byte half is a granule on
// its own (carries its tag), so the pair needs no atomicity beyond the naturally aligned 8 bytes.
__device__ __forceinline__ void gran2_store(rsrc_t r, unsigned byte_off, unsigned v0, unsigned v1, unsigned tag) {
  __builtin_amdgcn_raw_buffer_store_b128(u32x4{v0, tag, v1, tag}, r, (int)byte_off, 0, AUX_SC1);
}
__device__ __forceinline__ u32x4 gran2_load(rsrc_t r, unsigned byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, AUX_SC1);
}
// `local` (uniform): all slices of the batch group were found on ONE XCD (group_on_one_xcd below).  A plain store then KEEPS
// the line in that XCD's L2 and the siblings' sc1 (L1-bypassing) polls hit it there; an sc1 store drops the line from L2 and
// every poll pays the fabric round trip (MI355X_MICROARCH.md, "stores of each flavour").
__device__ __forceinline__ void gran2_publish(rsrc_t r, unsigned byte_off, unsigned v0, unsigned v1, unsigned tag, bool local) {
  if (local)
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{v0, tag, v1, tag}, r, (int)byte_off, 0, 0);
  else
    __builtin_amdgcn_raw_buffer_store_b128(u32x4{v0, tag, v1, tag}, r, (int)byte_off, 0, AUX_SC1);
}

__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
  const bf16_t x = (bf16_t)a, y = (bf16_t)b;
  return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ float bf16_lo(unsigned w) { return __builtin_bit_cast(float, w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __builtin_bit_cast(float, w & 0xffff0000u); }

// Gather CNT 16-byte granule pairs (bit k of `want`: this thread needs pair k at byte offset base + off[k]; the other offsets must
// still point into the workspace); a pair is accepted when both of its tags equal `tag`.  Every sweep issues ALL its loads before
// it looks at any of them: with a load inside the per-pair branch the compiler put `s_waitcnt vmcnt(0)` behind each one (seen in
// the ISA) and a 5-pair sweep paid five L2 round trips in a row.  The wave leaves together.  Returns false on timeout.
template <int CNT>
__device__ __forceinline__ bool gather_pairs(rsrc_t rx, const unsigned (&off)[CNT], unsigned base, unsigned want, unsigned tag,
                                             u32x4 (&v)[CNT]) {
  unsigned need = want;
  for (unsigned spins = 0;; ++spins) {
    u32x4 t[CNT];
#pragma unroll
    for (int k = 0; k < CNT; ++k) t[k] = gran2_load(rx, base + off[k]);
    __builtin_amdgcn_sched_barrier(0);       // (the scheduler otherwise sinks the last load behind the first wait)
#pragma unroll
    for (int k = 0; k < CNT; ++k) {
      if (((need >> k) & 1u) && t[k][1] == tag && t[k][3] == tag) {
        v[k] = t[k];
        need &= ~(1u << k);
      }
    }
    if (__all(need == 0)) return true;
    if (spins > SPIN_LIMIT) return false;
    __builtin_amdgcn_s_sleep(1);
  }
}

// Are the GROUP slices of this batch group on one XCD?  The block maps (persist_roles, decode_roles) rest on a dispatch-order
// ASSUMPTION, so it is verified per launch: every workgroup publishes its HW_REG_XCC_ID (sc1 store: visible anywhere) at
// hello_base + 16 g and reads its siblings' (lanes below GROUP, skipping g).  Only if all agree does this workgroup publish with
// plain stores.  A sibling that does not answer within SPINS polls counts as "elsewhere" (sc1 stores are always correct).  `sh`
// is one LDS word; status word PERSIST_ST_COLOCATED counts the workgroups that answered yes.  The two bounds in use (2^16 polls
// for the LSTM's 4 slices, SPIN_LIMIT for the decoder's 32) are inherited from the two files this came from; they were never
// measured against each other.
template <int GROUP, unsigned SPINS>
__device__ __forceinline__ bool group_on_one_xcd(rsrc_t rx, unsigned hello_base, int g, int xmap, int* sh, unsigned* status) {
  static_assert(GROUP <= 64, "one lane per sibling");
  if (!xmap) return false;
  unsigned me;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(me));
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid == 0) gran2_store(rx, hello_base + (unsigned)(g * 16), me, me, HELLO_TAG);
  if (tid < 64) {
    bool same = true;
    if (lane < GROUP && lane != g) {
      same = false;
      for (unsigned spins = 0; spins < SPINS; ++spins) {
        const u32x4 v = gran2_load(rx, hello_base + (unsigned)(lane * 16));
        if (v[1] == HELLO_TAG) { same = v[0] == me; break; }
        __builtin_amdgcn_s_sleep(2);
      }
    }
    const bool all_same = __all(same);
    if (lane == 0) {
      *sh = all_same ? 1 : 0;
      if (all_same) atomicAdd(status + PERSIST_ST_COLOCATED, 1u);
    }
  }
  __syncthreads();
  return *sh != 0;
}

// ---- host side: the workspace of one launch
struct PersistWs {
  u64* xch;             // the granule slots (= the workspace)
  unsigned hello_off;   // byte offset (from xch) of the XCC-id exchange
  unsigned* status;     // the status block
};

inline long long persist_ws_total(long long slot_bytes, long long hello_bytes) {
  return slot_bytes + hello_bytes + PERSIST_STATUS_BYTES;
}

// What every launcher does with (ws, ws_bytes): a NEGATIVE size means the caller already zeroed the buffer; the size is checked
// against the layout; unless prezeroed the whole buffer is zeroed on `stream` ahead of the launch.  `who` names the C entry point
// in the error texts.
inline int persist_ws_prepare(const char* who, void* ws, long long ws_bytes_signed, long long slot_bytes, long long hello_bytes,
                              hipStream_t stream, PersistWs* out) {
  const bool prezeroed = ws_bytes_signed < 0;
  const long long ws_bytes = prezeroed ? -ws_bytes_signed : ws_bytes_signed, need = persist_ws_total(slot_bytes, hello_bytes);
  MR_CHECK_ARG(ws_bytes >= need, "%s: workspace too small (%lld < %lld)", who, ws_bytes, need);
  if (!prezeroed && hipMemsetAsync(ws, 0, (size_t)need, stream) != hipSuccess) {
    set_error("%s: memset of the exchange buffer failed", who);
    return MR_ERR_LAUNCH;
  }
  *out = PersistWs{(u64*)ws, (unsigned)slot_bytes, (unsigned*)((char*)ws + slot_bytes + hello_bytes)};
  return MR_OK;
}

}  // namespace mr
