// All-taps weight-gradient kernel for 3x3 / stride 1 / "same" convolutions (bf16): interface between tn_taps.hip
// (kernel + launcher) and gemm_conv.hip (the mr_conv2d_wgrad_tab entry point that dispatches to it).
#pragma once
#include "common.h"

namespace mr {

// Geometry of one launch.  dw[k][r][s][c] += sum_{n,h,w} dy[n,h,w,k] * x[n, h+(r-1)*d, w+(s-1)*d, c]
struct TapsProblem {
  const void* dy;   // [N*H*W][lddy] bf16
  const void* x;    // [N*H*W][ldx] bf16
  float* dw;        // [Cout][3][3][Cin] f32, accumulated atomically
  float* dbias;     // optional [Cout]: += column sums of dy
  int* tab;         // caller-owned table, >= taps_table_ints(...) ints
  int build;        // != 0: fill the table first
  bool beside;      // the launch may run beside TN launches of another stream: it must not touch the shared workspace
  int N, H, W, Cin, ldx, Cout, lddy, dil;
};

// != 0 when the all-taps kernel can serve the geometry AND its stream table fits in `tab_bytes` bytes.
int taps_eligible(int N, int H, int W, int Cin, int ldx, int Cout, int lddy, int R, int S, int sh, int sw, int ph,
                  int pw, int dh, int dw, int Ho, int Wo, long long tab_bytes);
// Workspace of the in-launch group reduction (tickets + slabs; see TapArgs.grp): caller-owned device memory, zeroed
// once by the caller; launches that use it must be stream-ordered with respect to each other.
void taps_set_workspace(void* p, long long bytes);
void taps_get_workspace(void** p, long long* bytes);   // the current device's registered workspace (or null, 0)
#ifdef MR_ABLATION
int taps_set_abl(int mask);   // timing-only ablations (wrong results), see tn_taps.hip
#endif
int launch_tn_taps(const TapsProblem& p, int splits_override, hipStream_t stream);

// ---- recorded problems (mr_tn_defer / mr_tn_flush): several problems per launch, so that the workgroup slots of the chip are
// filled by problems, not by splits, and the fixed price of a workgroup is paid once per slot instead of once per layer.
constexpr int TAPS_PLAN_MAX = 12;   // problems per plan
int taps_build_table(const TapsProblem& p, hipStream_t stream);   // what p.build != 0 does, for a problem that is recorded
// Launches p[0..n) (tables built, n <= TAPS_PLAN_MAX) as taps_plan partitions them; a problem alone in its launch goes through
// launch_tn_taps.  p[i].build / p[i].beside are ignored: `beside` is the flush's.
int launch_tn_taps_group(const TapsProblem* p, int n, bool beside, hipStream_t stream);
// Host only.  Partitions n problems (tiles[i] output tiles of 64 Cout x 64 Cin x 9 taps, chunks[i] 64-position chunks to
// reduce) into launches on a chip of `cus` CUs with `slabs` partial-tile slabs in the workspace (0: none, atomics only) and
// cuts each into splits[i] workgroups of cps[i] chunks per tile.  Model, in chunk-times, summed over the launches:
// ceil(sum tiles * splits / (2 * cus)) * (largest cps of the launch + a fixed price per workgroup).  Up to 8 problems every
// partition is tried, above that problems are merged greedily in recording order.  launch[i] = launch index of problem i
// (0 .. launches-1, numbered by their first problem).  Returns the modelled cost, < 0 on bad arguments.
double taps_plan(int cus, int slabs, int n, const int* tiles, const int* chunks, int* launch, int* splits, int* cps);
double taps_plan_cost(int cus, int n, const int* tiles, const int* launch, const int* splits, const int* cps);

}  // namespace mr
