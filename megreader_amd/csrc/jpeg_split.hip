// Parallel decode inside ONE work item of the JPEG decoder (include/megreader_hip.h: mr_jpeg_plan_split, mr_jpeg_decode_split):
// a photo without restart markers is a single Huffman stream, which csrc/jpeg.hip decodes with one wavefront.  Here the item is
// cut into sub-sequences of S unstuffed bytes and every lane decodes one (self-synchronising sub-sequence decoding).
//
// The serial decoder's state BETWEEN two symbols is (p, b, k): bit position, block slot inside the MCU (it selects the DC/AC table
// pair), zigzag index (0: the next symbol is a DC size).  step() is the serial kernel's rule as a total function -- an invalid
// code takes 16 bits and yields symbol 0, the DC size is masked to 4 bits, a run past 63 ends the block, bits past the end are
// zero -- and every symbol takes at least one bit.  F_i(state) = "step while p < end_i", end_i = min((i + 1) * S, U) * 8 with U
// the item's unstuffed bytes (the identity when p >= end_i already).  The exact entry states are in[0] = (0, 0, 0),
// in[i + 1] = F_i(in[i]).
//
// WHY THE ENTRY STATES ARE EXACT.  Lane i starts from the guess (i * S * 8, 0, 0) and keeps two records: in[i], the state it was
// LAST DECODED FROM, and exit[i] = F_i(in[i]).  A lane is re-decoded exactly when in[i] != exit[i - 1].  The stages below end
// with the chain condition  in[0] = (0, 0, 0)  and  in[i] == exit[i - 1] for every i > 0  established, not assumed:
//   * inside a workgroup (256 consecutive sub-sequences, states in LDS) the rounds go on until __syncthreads_or reports that no
//     lane saw in[i] != exit[i - 1], or for `count` rounds, count = the workgroup's sub-sequences: lane 0's entry is fixed for
//     the launch, and round r makes lane r + 1 decode from the final exit of lane r, so after count - 1 rounds every lane has;
//   * across workgroups there are FURTHER LAUNCHES, never a wait: pass q hands workgroup g >= q the exit that workgroup g - 1
//     published in pass q - 1 (two copies by pass parity, so a pass reads only what the previous launch wrote).  Workgroup 0 is
//     exact after pass 0; if workgroups < q were exact after pass q - 1, workgroup q reads the exact exit of q - 1 in pass q,
//     re-decodes from it (or finds it equal to what it was decoded from and returns at once) and is exact.  The host enqueues
//     max(n_wg) - 1 further passes, known from the plan: the worst case, so nothing looks at the device.
// By induction over i, in[i] == exit[i - 1] == F_{i-1}(in[i - 1]) makes every in[i] the serial decoder's state, however slowly
// the guesses converged.  Every loop is bounded before it starts: S * 8 steps per sub-sequence (a step takes >= 1 bit and p never
// starts below i * S * 8), `count` rounds, n_wg - 1 passes, n_sub / 256 scan chunks.
//
// Stages (all launched between the status kernel and jpeg_color_kernel):
//   zero     the coefficient buffer;
//   unstuff  one workgroup per item drops the byte after every FF (as refill() of csrc/jpeg.hip does) into `raw`, zero behind;
//   sync     the passes above;
//   scan     block_off[i] = exclusive prefix sum of the blocks completed in sub-sequences < i; fewer than n_blocks: CORRUPT;
//   write    lane i decodes from in[i] once more and stores coefficients (zigzag order, DC as the DIFFERENCE) of blocks
//            < n_blocks; an invalid code, a DC size > 11 or a run past 63 inside such a block, or the last such block ending
//            behind the item's bits, is CORRUPT.  Blocks >= n_blocks (padding bits decode into them) are dropped silently, and
//            the speculative decodes of `sync` never touch the status;
//   dc       per component prefix sum of the DC differences in scan order;
//   idct     dequantise + inverse DCT, 8 blocks per wave with flush_blocks, into the planes the serial path fills.
#include <stddef.h>

#include "common.h"
#include "jpeg_idct.h"
#include "jpeg_plan.h"
#include "../../include/megreader_hip.h"

namespace mr {

using jpeg::Image;
using jpeg::Item;
using jpeg::Split;
using namespace jpeg_dev;

static_assert(sizeof(Split) == sizeof(mr_jpeg_split) && sizeof(Split) % 8 == 0, "csrc/jpeg_plan.h restates mr_jpeg_split");
static_assert(offsetof(Split, n_blocks) == offsetof(mr_jpeg_split, n_blocks) &&
              offsetof(Split, meta_off) == offsetof(mr_jpeg_split, meta_off) &&
              offsetof(Split, wg_exit_off) == offsetof(mr_jpeg_split, wg_exit_off) &&
              offsetof(Split, coef_bytes) == offsetof(mr_jpeg_split, coef_bytes), "csrc/jpeg_plan.h restates mr_jpeg_split");

namespace {

constexpr int WG = jpeg::SPLIT_WG;

struct State {
  unsigned p;   // bit position
  int b, k;     // block slot in the MCU, zigzag index
  int n;        // blocks completed since the state was adopted (not part of equality)
};

__device__ __forceinline__ uint2 pack(const State& s) { return make_uint2(s.p, (unsigned)s.n << 16 | (unsigned)s.b << 8 | (unsigned)s.k); }
__device__ __forceinline__ State unpack(uint2 v) {
  State s;
  s.p = v.x, s.n = (int)(v.y >> 16), s.b = (int)(v.y >> 8 & 255u), s.k = (int)(v.y & 255u);
  return s;
}
__device__ __forceinline__ bool same(uint2 a, uint2 b) { return a.x == b.x && ((a.y ^ b.y) & 0xFFFFu) == 0; }

// The image's Huffman tables in LDS.  lim[t][l]: the first 16-bit peek that is NOT a code of length <= l + 1 (the canonical
// codes of one length follow those of the shorter ones, so lim is non-decreasing and the code length is 1 + the number of l with
// peek >= lim[t][l]: the same length as the first l with (peek >> (15 - l)) <= maxcode[l], which is what the serial kernel takes).
struct Tables {
  int lim[4][16];
  int valoff[4][16];
  unsigned char syms[4 * 256];
};

__device__ __forceinline__ void load_tables(const Image* im, Tables& T, int t) {
  if (t < 4) {
    int prev = 0;
    for (int l = 0; l < 16; ++l) {
      const int mc = im->huff_maxcode[t * 16 + l];
      prev = mc >= 0 ? (mc + 1) << (15 - l) : prev;
      T.lim[t][l] = prev;
    }
  }
  if (t < 64) T.valoff[t >> 4][t & 15] = im->huff_valoff[t];
  for (int i = t; i < 256; i += WG) ((int*)T.syms)[i] = im->huff_sym[i];
  __syncthreads();
}

// What a lane needs to decode: the unstuffed bytes as words and the image's table selectors.
struct Dec {
  const unsigned* raw;
  unsigned last;   // the last word index a 64-bit read may start at
  int B, hsvs;
  int td[3], ta[3];
};

__device__ __forceinline__ Dec make_dec(const Image* im, const Split& sp, const unsigned char* ws) {
  Dec d;
  d.raw = (const unsigned*)(ws + sp.raw_off);
  d.last = (unsigned)(sp.raw_bytes / 4 - 2);
  d.B = sp.blocks_per_mcu;
  d.hsvs = im->ncomp == 3 ? im->hs * im->vs : 1;
#pragma unroll
  for (int c = 0; c < 3; ++c) d.td[c] = im->comp_td[c] & 1, d.ta[c] = im->comp_ta[c] & 1;
  return d;
}

__device__ __forceinline__ unsigned get32(const Dec& d, unsigned p) {   // the 32 bits from bit p on (zeros behind the data)
  const unsigned q = min(p >> 5, d.last);
  const unsigned long long v = (unsigned long long)__builtin_bswap32(d.raw[q]) << 32 | __builtin_bswap32(d.raw[q + 1]);
  return (unsigned)((v << (p & 31u)) >> 32);
}

__device__ __forceinline__ int extend(int v, int nbits) {   // T.81 F.2.2.1
  return nbits && v < (1 << (nbits - 1)) ? v - (1 << nbits) + 1 : v;
}

// One symbol from state s.  WRITE: the value goes to block `blk` when that is one of the item's n_blocks, and only then can
// the step be an error.  Returns true when the step completed a block.
template <bool WRITE>
__device__ __forceinline__ bool step(State& s, const Dec& d, const Tables& T, int blk, int n_blocks, int* dc, short* coef,
                                     bool& bad) {
  const unsigned w = get32(d, s.p);
  const int c = s.b < d.hsvs ? 0 : min(s.b - d.hsvs + 1, 2);
  const int t = s.k == 0 ? d.td[c] : 2 + d.ta[c];
  const int peek = (int)(w >> 16);
  int len = 1;
#pragma unroll
  for (int l = 0; l < 16; ++l) len += peek >= T.lim[t][l] ? 1 : 0;
  const bool invalid = len == 17;            // no length accepts these 16 bits: 16 bits, symbol 0
  len = min(len, 16);
  const int sym = invalid ? 0 : T.syms[t * 256 + (((peek >> (16 - len)) + T.valoff[t][len - 1]) & 255)];
  const unsigned rest = len == 16 ? w << 16 : w << len;
  bool err = invalid, done = false;
  int use = len, val = 0, at = -1;
  if (s.k == 0) {
    int size = sym;
    err |= size > 11;
    size &= 15;
    val = extend(size ? (int)(rest >> (32 - size)) : 0, size);
    use += size;
    at = 0;
    s.k = 1;
  } else {
    const int run = sym >> 4, nbits = sym & 15;
    if (nbits == 0) {
      if (run != 15) {
        done = true;
      } else {
        s.k += 16;
        done = s.k >= 64;
      }
    } else {
      s.k += run;
      if (s.k > 63) {
        err = done = true;
      } else {
        val = extend((int)(rest >> (32 - nbits)), nbits);
        use += nbits;
        at = s.k;
        done = ++s.k == 64;
      }
    }
  }
  s.p += (unsigned)use;
  if (WRITE && blk < n_blocks) {
    if (at == 0) dc[blk] = val;
    if (at > 0) coef[(long long)blk * 64 + at] = (short)val;
    bad |= err;
  }
  if (done) {
    s.k = 0;
    s.b = s.b + 1 == d.B ? 0 : s.b + 1;
    s.n += 1;
  }
  return done;
}

__device__ __forceinline__ unsigned end_of(const Split& sp, int i, unsigned nbits) {
  return min((unsigned)(i + 1) * (unsigned)sp.subseq_bytes * 8u, nbits);
}

// F_i without side effects: at most subseq_bytes * 8 steps.
__device__ __forceinline__ State advance(State s, const Dec& d, const Tables& T, unsigned end, int max_steps) {
  bool bad = false;
  for (int it = 0; it < max_steps && s.p < end; ++it) step<false>(s, d, T, 0, 0, nullptr, nullptr, bad);
  return s;
}

// Inclusive sum over the workgroup's 256 lanes; `total` is the sum of all of them.
__device__ __forceinline__ int wg_scan(int v, int* wsum, int t, int& total) {
  const int lane = t & 63, w = t >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int n = __shfl_up(v, o, 64);
    if (lane >= o) v += n;
  }
  __syncthreads();
  if (lane == 63) wsum[w] = v;
  __syncthreads();
  int add = 0, tot = 0;
#pragma unroll
  for (int j = 0; j < WG / 64; ++j) {
    add += j < w ? wsum[j] : 0;
    tot += wsum[j];
  }
  total = tot;
  return v + add;
}

// grid (256, split): the coefficient buffer, 16 bytes per store.
__global__ __launch_bounds__(WG) void jpeg_split_zero_kernel(const Image* images, const Split* splits, unsigned char* ws) {
  const Split& sp = splits[blockIdx.y];
  if (images[sp.image].status != jpeg::OK) return;
  uint4* dst = (uint4*)(ws + sp.coef_off);
  const long long n = sp.coef_bytes / 16;
  for (long long i = blockIdx.x * (long long)WG + threadIdx.x; i < n; i += (long long)gridDim.x * WG) dst[i] = make_uint4(0, 0, 0, 0);
}

// grid (split): a byte of the item is kept unless the byte in front of it, inside the item, is FF.  16 source bytes per lane and
// round (aligned: the blob buffer and blob_off are 16-byte aligned and every blob is padded to 16), positions by a workgroup scan.
__global__ __launch_bounds__(WG) void jpeg_split_unstuff_kernel(const unsigned char* blobs, const Image* images, const Item* items,
                                                                const Split* splits, unsigned char* ws) {
  __shared__ int wsum[WG / 64];
  const Split& sp = splits[blockIdx.x];
  const Image* im = images + sp.image;
  if (im->status != jpeg::OK) return;
  const int t = threadIdx.x;
  const Item it = items[sp.item];
  const unsigned char* base = blobs + im->blob_off;
  const long long begin = it.off, end = it.off + it.len;
  unsigned char* raw = ws + sp.raw_off;
  long long total = 0;
  for (long long chunk = begin & ~15LL; chunk < end; chunk += 16 * WG) {
    const long long p = chunk + 16 * t;
    uint4 v = make_uint4(0, 0, 0, 0);
    unsigned prev = 0;
    if (p < end) {
      v = *(const uint4*)(base + p);
      if (p > begin) prev = base[p - 1];
    }
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned keep = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const unsigned b = (w[j >> 2] >> (8 * (j & 3))) & 255u;
      if (p + j >= begin && p + j < end && !(p + j > begin && prev == 255u)) keep |= 1u << j;
      prev = b;
    }
    int tot;
    const int cnt = __popc(keep);
    long long at = total + wg_scan(cnt, wsum, t, tot) - cnt;
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (keep >> j & 1u) raw[at++] = (unsigned char)((w[j >> 2] >> (8 * (j & 3))) & 255u);   // at < it.len <= raw_bytes - 16
    total += tot;
  }
  __syncthreads();
  for (long long q = total + t; q < sp.raw_bytes; q += WG) raw[q] = 0;
  if (t < 4) ((int*)(ws + sp.meta_off))[t] = t == 0 ? (int)total : 0;
}

// grid (largest n_wg - pass, split): workgroup g = blockIdx.x + pass of the item (the ones in front are final).
__global__ __launch_bounds__(WG) void jpeg_split_sync_kernel(const Image* images, const Split* splits, unsigned char* ws, int pass) {
  __shared__ Tables T;
  __shared__ uint2 lds_exit[WG];
  const Split& sp = splits[blockIdx.y];
  const int g = blockIdx.x + pass;
  if (g >= sp.n_wg) return;
  const Image* im = images + sp.image;
  if (im->status != jpeg::OK) return;
  const int t = threadIdx.x, i = g * WG + t;
  const int count = min(WG, sp.n_sub - g * WG);
  const bool valid = t < count;
  uint2* in_g = (uint2*)(ws + sp.in_off);
  uint2* exit_g = (uint2*)(ws + sp.exit_off);
  uint2* wg_cur = (uint2*)(ws + sp.wg_exit_off) + (pass & 1) * sp.n_wg;
  const uint2* wg_prev = (const uint2*)(ws + sp.wg_exit_off) + ((pass & 1) ^ 1) * sp.n_wg;
  uint2 handed = make_uint2(0, 0);
  if (pass > 0) {   // g >= 1
    handed = wg_prev[g - 1];
    if (same(handed, in_g[g * WG])) {   // decoded from exactly this state already: its exit stands
      if (t == 0) wg_cur[g] = wg_prev[g];
      return;
    }
  }
  load_tables(im, T, t);
  const Dec d = make_dec(im, sp, ws);
  const unsigned nbits = (unsigned)((const int*)(ws + sp.meta_off))[0] * 8u;
  const int max_steps = sp.subseq_bytes * 8;
  const unsigned end = end_of(sp, i, nbits);
  State in = {0u, 0, 0, 0}, ex = {0u, 0, 0, 0};
  if (valid) {
    if (pass == 0) {
      in.p = (unsigned)i * (unsigned)sp.subseq_bytes * 8u;   // the guess; for i == 0 the true start
      ex = advance(in, d, T, end, max_steps);
    } else {
      in = unpack(in_g[i]), ex = unpack(exit_g[i]);
      if (t == 0) {
        in = unpack(handed), in.n = 0;
        ex = advance(in, d, T, end, max_steps);
      }
    }
  }
  lds_exit[t] = pack(ex);
  for (int r = 0; r < count; ++r) {
    __syncthreads();
    bool changed = false;
    uint2 pv = make_uint2(0, 0);
    if (valid && t > 0) {
      pv = lds_exit[t - 1];
      changed = !same(pv, pack(in));
    }
    if (!__syncthreads_or(changed)) break;   // (also the barrier between the reads above and the writes below)
    if (changed) {
      in = unpack(pv), in.n = 0;
      ex = advance(in, d, T, end, max_steps);
      lds_exit[t] = pack(ex);
    }
  }
  if (valid) {
    in_g[i] = pack(in);
    exit_g[i] = pack(ex);
    if (t == count - 1) wg_cur[g] = pack(ex);
  }
}

// grid (split): block_off and the number of completed blocks.
__global__ __launch_bounds__(WG) void jpeg_split_scan_kernel(const Image* images, const Split* splits, unsigned char* ws, int* status) {
  __shared__ int wsum[WG / 64];
  const Split& sp = splits[blockIdx.x];
  if (images[sp.image].status != jpeg::OK) return;
  const int t = threadIdx.x;
  const uint2* exit_g = (const uint2*)(ws + sp.exit_off);
  int* block_off = (int*)(ws + sp.block_off);
  int carry = 0;
  for (int base = 0; base < sp.n_sub; base += WG) {
    const int i = base + t;
    const int v = i < sp.n_sub ? (int)(exit_g[i].y >> 16) : 0;
    int tot;
    const int incl = wg_scan(v, wsum, t, tot);
    if (i < sp.n_sub) block_off[i] = carry + incl - v;
    carry += tot;
  }
  if (t == 0) {
    ((int*)(ws + sp.meta_off))[1] = carry;
    if (carry < sp.n_blocks) atomicMax(status + sp.image, (int)jpeg::CORRUPT);
  }
}

// grid (ceil(largest n_sub / 256), split): every lane decodes its sub-sequence from its exact entry state.
__global__ __launch_bounds__(WG) void jpeg_split_write_kernel(const Image* images, const Split* splits, unsigned char* ws, int* status) {
  __shared__ Tables T;
  const Split& sp = splits[blockIdx.y];
  if ((int)blockIdx.x * WG >= sp.n_sub) return;
  const Image* im = images + sp.image;
  if (im->status != jpeg::OK) return;
  const int t = threadIdx.x, i = blockIdx.x * WG + t;
  load_tables(im, T, t);
  if (i >= sp.n_sub) return;
  const int base = ((const int*)(ws + sp.block_off))[i];
  if (base >= sp.n_blocks) return;   // only dropped blocks from here on
  const Dec d = make_dec(im, sp, ws);
  const unsigned nbits = (unsigned)((const int*)(ws + sp.meta_off))[0] * 8u;
  const unsigned end = end_of(sp, i, nbits);
  int* dc = (int*)(ws + sp.coef_off);
  short* coef = (short*)(ws + sp.coef_off + ((4LL * sp.n_blocks + 15) & ~15LL));
  State s = unpack(((const uint2*)(ws + sp.in_off))[i]);
  s.n = 0;
  bool bad = false;
  const int max_steps = sp.subseq_bytes * 8;
  for (int it = 0; it < max_steps && s.p < end; ++it) {
    const int blk = base + s.n;
    const bool done = step<true>(s, d, T, blk, sp.n_blocks, dc, coef, bad);
    if (done && blk == sp.n_blocks - 1 && s.p > nbits) bad = true;   // the item ended inside its last block
  }
  if (bad) atomicMax(status + sp.image, (int)jpeg::CORRUPT);
}

// grid (split): DC differences -> DC values, per component in scan order; 256 MCUs per round.
__global__ __launch_bounds__(WG) void jpeg_split_dc_kernel(const Image* images, const Split* splits, unsigned char* ws) {
  __shared__ int wsum[WG / 64];
  const Split& sp = splits[blockIdx.x];
  const Image* im = images + sp.image;
  if (im->status != jpeg::OK) return;
  const int t = threadIdx.x, B = sp.blocks_per_mcu, nmcu = sp.n_blocks / B;
  const int ny = B == 1 ? 1 : B - 2;
  int* dc = (int*)(ws + sp.coef_off);
  int carry[3] = {0, 0, 0};
  for (int m0 = 0; m0 < nmcu; m0 += WG) {
    const int m = m0 + t;
    const bool live = m < nmcu;
    int* mine = dc + (long long)(live ? m : 0) * B;
    int sum[3] = {0, 0, 0};
    if (live) {
      for (int j = 0; j < ny; ++j) sum[0] += mine[j];
      if (B > 1) sum[1] = mine[ny], sum[2] = mine[ny + 1];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c > 0 && B == 1) break;
      int tot;
      const int incl = wg_scan(sum[c], wsum, t, tot);
      if (live) {
        if (c == 0) {
          int run = carry[0] + incl - sum[0];
          for (int j = 0; j < ny; ++j) mine[j] = run += mine[j];
        } else {
          mine[ny + c - 1] = carry[c] + incl;
        }
      }
      carry[c] += tot;
    }
  }
}

// grid (ceil(largest n_blocks / 8), split), one wave: dequantise 8 blocks into LDS (lane k places coefficient k) and flush them.
__global__ __launch_bounds__(64) void jpeg_split_idct_kernel(const Image* images, const Item* items, const Split* splits,
                                                             unsigned char* ws) {
  __shared__ __attribute__((aligned(16))) int blk[8 * BLK_STRIDE];
  __shared__ long long slot_dst[8];
  __shared__ int slot_pitch[8];
  const Split& sp = splits[blockIdx.y];
  const int j0 = blockIdx.x * 8;
  if (j0 >= sp.n_blocks) return;
  const Image* im = images + sp.image;
  if (im->status != jpeg::OK) return;
  const int lane = threadIdx.x, ns = min(8, sp.n_blocks - j0), B = sp.blocks_per_mcu, mcu_w = im->mcu_w;
  const int mcu0 = items[sp.item].mcu0;
  const int* dc = (const int*)(ws + sp.coef_off);
  const short* coef = (const short*)(ws + sp.coef_off + ((4LL * sp.n_blocks + 15) & ~15LL));
  const int ny = B == 1 ? 1 : B - 2, at = ZIGZAG[lane];
  for (int bb = 0; bb < ns; ++bb) {
    const int j = j0 + bb, m = mcu0 + j / B, slot = j % B;
    const int c = slot < ny ? 0 : slot - ny + 1;
    const int hs = c == 0 ? im->hs : 1, vs = c == 0 ? im->vs : 1, sub = c == 0 ? slot : 0;
    const int my = m / mcu_w, mx = m - my * mcu_w, by = sub / hs, bx = sub - by * hs;
    const int pitch = im->plane_pitch[c];
    const int q = ((const unsigned char*)im->quant)[64 * (im->comp_tq[c] & 3) + lane];
    const int v = lane == 0 ? dc[j] : (int)coef[(long long)j * 64 + lane];
    blk[bb * BLK_STRIDE + at] = v * q;
    if (lane == 0) {
      slot_dst[bb] = im->plane_off[c] + (long long)(my * vs + by) * 8 * pitch + (mx * hs + bx) * 8;
      slot_pitch[bb] = pitch;
    }
  }
  flush_blocks(blk, slot_dst, slot_pitch, ns, ws, lane);
}

}  // namespace

// The split stages of mr_jpeg_decode_split, enqueued on `stream` behind the status kernel.
int jpeg_split_stages(const unsigned char* blobs, const Image* images, const Item* items, const Split* host, const Split* dev,
                      int n_splits, unsigned char* ws, int* status, hipStream_t stream) {
  int max_wg = 0, max_sub = 0, max_blocks = 0;
  for (int i = 0; i < n_splits; ++i) {
    const Split& s = host[i];
    MR_CHECK_ARG(s.subseq_bytes >= 16 && s.subseq_bytes <= 1024 && s.subseq_bytes % 4 == 0 && s.n_sub > 0 &&
                     s.n_wg == cdiv(s.n_sub, WG) && s.n_blocks > 0 && s.blocks_per_mcu > 0 &&
                     s.raw_bytes >= (long long)s.n_sub * s.subseq_bytes + 16,
                 "mr_jpeg_decode_split: split %d is not what mr_jpeg_plan_split writes", i);
    max_wg = s.n_wg > max_wg ? s.n_wg : max_wg;
    max_sub = s.n_sub > max_sub ? s.n_sub : max_sub;
    max_blocks = s.n_blocks > max_blocks ? s.n_blocks : max_blocks;
  }
  hipLaunchKernelGGL(jpeg_split_zero_kernel, dim3(256, n_splits), dim3(WG), 0, stream, images, dev, ws);
  hipLaunchKernelGGL(jpeg_split_unstuff_kernel, dim3(n_splits), dim3(WG), 0, stream, blobs, images, items, dev, ws);
  for (int pass = 0; pass < max_wg; ++pass)
    hipLaunchKernelGGL(jpeg_split_sync_kernel, dim3(max_wg - pass, n_splits), dim3(WG), 0, stream, images, dev, ws, pass);
  hipLaunchKernelGGL(jpeg_split_scan_kernel, dim3(n_splits), dim3(WG), 0, stream, images, dev, ws, status);
  hipLaunchKernelGGL(jpeg_split_write_kernel, dim3(cdiv(max_sub, WG), n_splits), dim3(WG), 0, stream, images, dev, ws, status);
  hipLaunchKernelGGL(jpeg_split_dc_kernel, dim3(n_splits), dim3(WG), 0, stream, images, dev, ws);
  hipLaunchKernelGGL(jpeg_split_idct_kernel, dim3(cdiv(max_blocks, 8), n_splits), dim3(64), 0, stream, images, items, dev, ws);
  MR_CHECK_LAUNCH();
  return MR_OK;
}

}  // namespace mr

using namespace mr;

extern "C" {

int mr_sizeof_jpeg_split(void) { return (int)sizeof(mr_jpeg_split); }

int mr_jpeg_plan_split(int n_images, const mr_jpeg_image* images, mr_jpeg_item* items, long long n_items, long long split_above,
                       int subseq_bytes, mr_jpeg_split* splits, long long max_splits, long long* totals, long long* n_splits) {
  MR_CHECK_ARG(n_images >= 0 && n_items >= 0 && max_splits >= 0 && split_above >= 0 && totals != nullptr && n_splits != nullptr,
               "mr_jpeg_plan_split: bad arguments n_images=%d n_items=%lld max_splits=%lld split_above=%lld", n_images, n_items,
               max_splits, split_above);
  MR_CHECK_ARG(subseq_bytes >= 16 && subseq_bytes <= 1024 && subseq_bytes % 4 == 0,
               "mr_jpeg_plan_split: subseq_bytes=%d is not a multiple of 4 in [16, 1024]", subseq_bytes);
  MR_CHECK_ARG(n_items == 0 || (images != nullptr && items != nullptr), "mr_jpeg_plan_split: null pointer");
  MR_CHECK_ARG(max_splits == 0 || splits != nullptr, "mr_jpeg_plan_split: null split table");
  for (long long i = 0; i < n_items; ++i)
    MR_CHECK_ARG(items[i].image >= 0 && items[i].image < n_images, "mr_jpeg_plan_split: item %lld names image %d", i, items[i].image);
  *n_splits = jpeg::plan_split((const Image*)images, (Item*)items, n_items, split_above, subseq_bytes, (Split*)splits, max_splits,
                               &totals[2]);
  return MR_OK;
}

}  // extern "C"
