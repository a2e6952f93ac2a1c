/* megreader_hip.h -- C ABI of libmegreader_hip.so (MI355X / gfx950 kernels for MegReader's training hot path).
 *
 * Every entry point takes raw device pointers, plain sizes and a hipStream_t; no torch types cross this
 * boundary.  The library owns no tensors: the caller allocates every output and scratch buffer (its only state
 * is one 4 KiB zero page per device, the source of padded vectors for direct-to-LDS loads).  All functions return 0 on success and a non-zero MR_ERR_* code otherwise; mr_last_error() returns
 * a human-readable message for the calling thread.  Kernels are enqueued on `stream` and never synchronise.
 *
 * dtype codes: 0 = float32, 1 = bfloat16 (storage type of activations / operand images; accumulation is
 * always float32, CTC recursions float64).
 *
 * Layout conventions: activations NHWC (channel contiguous), convolution weights KRSC, matrices row-major.
 * "16-byte vector" = 4 float32 or 8 bfloat16; channel counts and leading dimensions of MFMA operands must
 * be multiples of one vector.
 *
 * Each group cites the reference interface (file:line in Megvii-CSG/MegReader) it replaces.
 */
#ifndef MEGREADER_HIP_H
#define MEGREADER_HIP_H

#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MR_ABI_VERSION 3   /* 3 (round 6): mr_tuning grew (nt_m32, nt_m32_opt, reserved[3]).  2 (round 5): mr_ctc_fwd gained log_probs_f64; mr_tuning.tn_defer; mr_tn_defer / mr_tn_flush;
                              the 26 mr_set_* setters of version 1 are gone (mr_tuning) */
#define MR_DTYPE_F32 0
#define MR_DTYPE_BF16 1

const char* mr_last_error(void);
int mr_abi_version(void);
/* Measurement only (bench.py's roofline pass): while mr_phase_timer(1) is in force, entry points made of several launches (the
 * DCNv2 forward / backward) bracket their parts with HIP events on the launch stream; mr_phase_read(id, &ms, &work) waits for them
 * and returns the number of records of phase id with their total milliseconds and total algorithmic work (bytes for the
 * bandwidth-bound passes, flops for the GEMMs).  ids: 0 dcn forward, 1 gcol GEMM, 2 coordinate pass, 3 CSR build (4 launches),
 * 4 input-gradient gather, 5 im2col, 6 weight-gradient GEMM.  Not capturable.  Host only. */
int mr_phase_timer(int on);
int mr_phase_read(int id, double* total_ms, double* total_work);
/* creates the per-device zero page eagerly and applies MEGREADER_TUNING (below); call before hipGraph capture */
int mr_init(void);

/* ---- Tuning / A-B state: ONE struct -----------------------------------------------------------------------------------------
 * Everything in the library that is process-wide and mutable, apart from the per-device zero page and the registered split-
 * reduction workspace, is this struct.  Rounds 1-3 exported 26 separate `mr_set_*` functions over 26 unsynchronised globals;
 * they are gone.  Every field selects between kernels that compute the SAME result (test / A-B / tuning hooks; the defaults are
 * what bench.py measures); the timing-only ablations that compute wrong results exist only in the -DMR_ABLATION tools build
 * (include/megreader_hip_ablation.h).
 *   mr_tuning_get / mr_tuning_set  read / replace the whole struct (writers serialised by a mutex, values range-checked);
 *   MEGREADER_TUNING="field=value,field=value"  is applied once by mr_init().
 * Threading: the compute entry points may be called from any thread on any stream; each of them reads the fields it needs with
 * single atomic loads, so a call that races with mr_tuning_set sees, per field, either the old or the new value -- never garbage.
 * Flipping fields while a training step is in flight is still only meaningful for A/B measurements. */
typedef struct mr_tuning {
  int nt_variant;    /* 2 (default) = direct-to-LDS NT kernels, 1 = register-staged NT kernel */
  int nt_deep;       /* pipeline depth of the 4-wave direct-to-LDS NT kernel: 1 (default) = launches with at most ~1.5 workgroups
                        per CU and >= 8 k-steps (bf16) run with 4 LDS stage buffers and 3 k-steps of LDS-DMA in flight across raw
                        barriers; 0 = always the 2-buffer loop; 2 = always the 4-buffer loop.  Same results bit for bit */
  int nt_big;        /* 8-wave big-tile NT kernels (256x256 / 272x256 / 288x128): 0 automatic, -1 never, 1..13 forced variants */
  int nt_p8;         /* 1 = phased-schedule 256x256 NT kernel (igemm_p8.h) for the big-tile launches, 0 (default) = plain */
  int nt_force_bm;   /* force one 4-wave NT tile shape: bm in {128, 96, 64} with */
  int nt_force_bn;   /* bn in {128, 64}; bm = 0 (default) = the cost model */
  int gemm_skinny;   /* 1 (default): M <= 32 GEMMs (attention decode loop) take the latency-optimised kernel of gemm_skinny.hip */
  int tn_big;        /* experimental wide-tile TN (weight-gradient) kernels: 1 = 256x256, 2 = 128x256, 0 / -1 = never (default) */
  int tn_buf;        /* TN operand staging: 1 (default) = raw buffer resources (out-of-range -> zeros), 0 = flat pointers */
  int tn_taps;       /* 1 (default): all-taps weight-gradient kernel for 3x3 / stride 1 / padding == dilation layers (tn_taps.hip)
                        through mr_conv2d_wgrad_tab; the row table has another format for it: rebuild tables after changing this */
  int tn_taps_group; /* split reduction of the all-taps kernel: 0 automatic, 1 atomics only, > 1 forced group size */
  int tn_group;      /* same for the 128x128 TN GEMM kernel (uses the same workspace) */
  int tn_fin;        /* 128x128 TN GEMM kernel: 2 = split partials -> slabs + finalize launch (measured slower), 0 (default) */
  int tn_taps_fin;   /* all-taps kernel: 0 (default) leaders' atomics; 1 group sums added by a finalize launch; 2 no in-launch
                        reduction, the finalize launch sums every split (1 and 2 measured within +-1 % of 0) */
  int tn_taps_w8;    /* 1: 8-wave workgroup variant of the all-taps kernel (one per CU, half the partial tiles) */
  int tn_model;      /* 1 (default): conv wgrad launches use the measured dense-GEMM split model */
  int tn_splits;     /* P-split override of the TN kernels, 0 (default) = the makespan model */
  int bn_fused;      /* 1 (default): BatchNorm finalisation folded into the apply passes (C % 64 == 0), 0 = separate launches */
  int lstm_persist;  /* 1 (default): persistent recurrence kernels (bf16, H = 256); 0 = one launch per step; 2 = persistent
                        without the XCD-colocating block map */
  int lstm_fwd_bn;   /* step kernels: hidden columns per workgroup forward (0 automatic, 32, 64) */
  int lstm_bwd_bn;   /* ... and backward (0 automatic, 16, 32 (default), 64) */
  int dcn_fused;     /* 1 (default): fused DCNv2 kernels (dcn_fused.hip) where the shape allows; 0 = the general kernels */
  int dcn_v1_bwd;    /* general DCN path: 1 (default) = round-1 backward kernels, 0 = the round-2 experiments */
  int bn_onepass;    /* 1 (default): BatchNorm backward of tensors that fit the registers of one resident grid runs as ONE launch
                        (reductions, a barrier among the workgroups of a 64-channel slab, dx from registers); 0 = always the
                        reduction launch + the apply launch */
  int skinny_depth;  /* k-chunks in flight per wave of the M <= 32 GEMM: 0 (default) = 4, or 8 when K needs more than one round
                        trip at 4 (K > 512 in bf16); 4 / 8 forced */
  int nt_big_min_k;  /* smallest K for which the automatic choice considers the 8-wave big-tile NT kernels (default 512) */
  int tn_taps_min_p; /* layers with fewer output pixels (N * H * W) than this (default 10000) keep the 128x128 TN GEMM kernel
                        instead of the all-taps kernel (round-4 in-step A/B: FPN-attention 9.68 -> 9.56 ms, CRNN at 32 crops per
                        GPU 1.47 -> 1.41, the P >= 16384 layers of Res50-PPM keep the all-taps kernel); rebuild row tables after
                        changing it (as for tn_taps) */
  int tn_defer;      /* 1 (default): mr_tn_defer(1) records the weight-gradient launches of the 128x128 TN GEMM kernel and
                        mr_tn_flush launches them several problems per launch (round 5); 0: mr_tn_defer is ignored, every
                        launch is immediate (A/B) */
  int pool_fixed;    /* 1 (default): max-pool forward with the window geometry as template constants (one packed store for the
                        arg-max codes) and the pooled-element-organised backward of the 2x2 / stride 2 pool (round 5); 0: the
                        round-4 kernels (bit-identical results; A/B) */
  int ctc_linear;    /* 1 (default): 1-D CTC recursions in the scaled linear domain (float64 products with exact power-of-two
                        rescaling, emission table in LDS) when the table fits; 0: the log-domain kernels (float64 log-sum-exp
                        per state and step).  alpha / beta buffers change meaning with it: the same value must be in force for
                        mr_ctc_fwd and the mr_ctc_bwd that consumes its buffers */
  int nt_wide8;      /* 8-wave workgroups (two per CU) instead of the 4-wave ones on the NT tile shapes named by this bit mask:
                        1 = 128x128, 2 = 128x64, 4 = 96x128, 8 = 64x128, 16 = 96x64, 32 = 64x64; 0 = never (round 4) */
  int nt_ksplit;     /* split reduction of the 4-wave NT kernels for launches of a few tiles with a long k-loop (round 5:
                        at most a quarter of the CUs busy, >= 16 k-steps): 1 (default) = as many splits as fill the chip once
                        with >= 4 k-steps each (<= 8), n > 1 = at most n, 0 = never.  Partial tiles meet in f32 slabs of the
                        split-reduction workspace (mr_set_tn_taps_workspace) and are added in split order: the same bits every
                        run; without a registered workspace the launch is unsplit.  Like the weight-gradient launches that use
                        that workspace, split launches must be stream-ordered with every other user of it: a process that
                        drives the library from two streams at once (training beside inference) sets this field to 0 */
  int nt_m32;        /* round 6: ping-pong NT kernel on v_mfma_f32_32x32x16_bf16 (nt32.hip: 8 waves as two groups one phase apart,
                        one always in its MFMA-only compute phase; output tile through LDS).  0 (default) = never: measured EQUAL
                        to the round-5 kernels on every CRNN layer (profiles/r06_nt32_*: the steady-state k-tile is 15 % shorter,
                        the fixed cost per launch 6 us longer; both kernels sit on the same launch + epilogue cost and the
                        chip's power-limited MFMA rate); 1 = wherever the automatic choice takes a 256-column big tile
                        (256x256 -> 256x256, 272x256 -> 288x256 as 1x8 waves); 2..5 = shape 256x256 / 288x256 / 256x128 / 128x256
                        for every eligible bf16 launch (sweeps) */
  int nt_m32_opt;    /* schedule variant of that kernel, 10 * PH + OPT (tools build -DMR_NT32_SWEEP only); 0 = the default */
  int dcn_gcol;      /* round 6: 1 (default) = bf16 DCNv2 backward through ONE materialised gcol = dy * W (tuned NT GEMM, bf16 output)
                        read by a coordinate-gradient pass and a CSR gather pass for the input gradient (dcn_fused.hip, C in
                        {64, 128, 256, 512}); 0 = the round-3 fused kernels (gcol in accumulators, gather-GEMM).  Changes the size
                        mr_dcn2_ws_bytes reports: workspaces must be sized under the value in force at the call */
  int dcn_col_fwd;   /* round 6: 1 (default) = on the dcn_gcol shapes the bf16 forward also goes through the column matrix (one sampling
                        pass into the caller's col_ws + the tuned NT GEMM) and leaves it there for the backward's weight gradient
                        (mr_dcn2_col_saved / mr_dcn2_bwd3); 0 = the fused forward kernel, the backward samples again */
  int decode_persist; /* round 6: 1 (default) = the attention-GRU decode loop runs its forward and its backward as ONE persistent launch
                        each (decode_persist.hip: bf16, H = 512, T <= 64, Ep <= 576; mr_decode_persist_ok); 0 = three launches per
                        step; 2 = persistent without the block map that puts a batch group's 32 workgroups on one XCD (A/B knob) */
  int reserved[3];   /* zero */
} mr_tuning;
int mr_tuning_get(mr_tuning* out);
int mr_tuning_defaults(mr_tuning* out);
int mr_tuning_set(const mr_tuning* in);   /* MR_ERR_ARG (mr_last_error names the field) when a value is out of range */

/* ---- GEMM family (replaces cuBLAS/cuDNN behind nn.Linear / nn.LSTM input projection:
 *      decoders/crnn.py:13-24; decoders/attention_decoder.py:187-231) ------------------------------------- */
/* C[M,N] = act(A[M,K] * B[N,K]^T + bias[N]);  A,B,C of `dtype`, bias f32 (nullable), relu 0/1 */
int mr_gemm_nt(int dtype, const void* A, long long lda, const void* B, int ldb, void* C, long long ldc,
               const float* bias, int relu, int M, int N, int K, hipStream_t stream);
/* M <= 32 problems (the decode-loop GEMMs of the attention decoder) take a latency-optimised kernel (csrc/gemm_skinny.hip:
 * 16 output columns per workgroup, K split over the four waves, operands fetched as MFMA fragments straight from global
 * memory) unless mr_tuning.gemm_skinny = 0. */
/* workspace of the all-taps kernel's in-launch split reduction: device memory zeroed once by the caller (16 KB of
 * tickets + 147456 B per workgroup of the largest launch = 2 * CUs slabs); NULL / 0 withdraws it (f32 atomics only).
 * Launches that use it must be stream-ordered with each other. */
int mr_set_tn_taps_workspace(void* ws, long long bytes);
/* host only: 1 when mr_conv2d_wgrad_tab (bf16, non-NULL row table) would run the all-taps kernel for this geometry
 * under the current mr_tuning.tn_taps setting */
int mr_tn_taps_would_run(int N, int H, int W, int Cin, int ldx, int Cout, int lddy, int R, int S, int sh, int sw,
                         int ph, int pw, int dh, int dw, int Ho, int Wo);
/* host only: how mr_tn_flush launches n <= 12 recorded all-taps problems on a chip of `cus` CUs whose workspace holds `slabs`
 * partial-tile slabs (0: atomics only).  tiles[i] = 64 x 64 x 9-tap output tiles, chunks[i] = 64-position chunks of the pixel
 * stream of problem i; out: launch[i] (launch index, numbered by first problem), splits[i] workgroups per tile, cps[i] chunks
 * per workgroup, *cost = the modelled cost in chunk-times: sum over the launches of ceil(sum tiles * splits / (2 * cus)) *
 * (largest cps + 12).  Every partition is tried for n <= 8, greedy merging in recording order above.  Returns the number of
 * launches, < 0 on bad arguments. */
int mr_tn_taps_plan(int cus, int slabs, int n, const int* tiles, const int* chunks, int* launch, int* splits, int* cps,
                    double* cost);
/* host only: how mr_tn_flush launches n <= 64 recorded problems of the 128x128 TN GEMM kernel, in recording order, on a chip of
 * `cus` CUs.  tiles[i] = 128 x 128 output tiles, steps[i] = 64-row p-steps of the reduction, modes[i] = 0 (dense B operand) or 2
 * (conv operand through a row table); both modes share a launch.  The records are cut into ceil(n / mr_tn_capacity(0)) runs of
 * equal length; a run is one launch, or one launch per mode where the model prices that lower (problems of very different depth).
 * out: launch[i] (numbered by first problem), splits[i] (workgroups per tile, each of ceil(steps / splits) p-steps, none empty), begin[i] (first
 * workgroup of problem i inside its launch, a multiple of 8; a problem owns tiles * splits workgroups rounded up to 8), *cost =
 * the modelled cost in dense p-steps: per launch ceil(workgroups / (2 * cus)) * (longest workgroup + 20) * (1.3 when workgroups
 * share CUs), a conv p-step counting 1.02 dense ones.  The splits are chosen per problem to minimise it.  A problem alone in
 * its launch is launched as an immediate call would launch it.  Plans are cached by their inputs.  Returns the number of
 * launches, < 0 on bad arguments. */
int mr_tn_group_plan(int cus, int n, const int* tiles, const int* steps, const int* modes, int* launch, int* splits, int* begin,
                     double* cost);
/* host only: *cost = the modelled cost (as above) of ONE launch of n problems cut into the given splits[i] <= steps[i] */
int mr_tn_group_cost(int cus, int n, const int* tiles, const int* steps, const int* modes, const int* splits, double* cost);
/* host only: problems per launch of mr_tn_flush; kind 0: the 128x128 TN GEMM kernel, kind 1: the all-taps kernel, else 0 */
int mr_tn_capacity(int kind);
/* tile (BM*1000+BN) the NT kernels pick for an M x N problem; host-only query used for profiling labels */
int mr_nt_tile_code(int M, int N);
/* same, including the big-tile policy (returns 256256 for the 8-wave 256x256 kernel); cg = channels of the gathered
 * conv operand, 0 for a dense GEMM */
int mr_nt_kernel_code(int dtype, int M, int N, int K, int cg);
/* C[NA,NB] (f32) += A[P,NA]^T * B[P,NB];  row_perm_h>0: gate-interleaved rows are written back in
 * PyTorch gate-major order (see lstm section).  colsum (nullable, f32[NA]) += sum_p A[p,:] (bias gradient,
 * fused into the same pass over A). */
int mr_gemm_tn(int dtype, const void* A, long long lda, const void* B, long long ldb, float* C, int ldc, int P,
               int NA, int NB, int row_perm_h, float* colsum, hipStream_t stream);
/* the same with a second destination for the column sums (colsum2, nullable; ignored when colsum is null): b_ih and b_hh of an
 * LSTM direction (decoders/crnn.py:13 nn.LSTM keeps both) receive the same gradient from one launch */
int mr_gemm_tn2(int dtype, const void* A, long long lda, const void* B, long long ldb, float* C, int ldc, int P,
                int NA, int NB, int row_perm_h, float* colsum, float* colsum2, hipStream_t stream);

/* Deferred, grouped weight-gradient launches (round 5).  The weight gradients of small layers -- the 1x1 / strided layers of a
 * ResNet at batch 32 (backbones/resnet.py:113-181), the LSTM / Linear layers of the CRNN head (decoders/crnn.py:8-24) -- are GEMMs
 * of 16..64 output tiles: alone, each has to cut its pixel loop into 8..32 splits to fill the chip.  Nothing later in the backward
 * pass reads them, so they can wait and run side by side.  mr_tn_defer(1): on the calling host thread, bf16 launches that would
 * take the 128x128 TN GEMM kernel (mr_gemm_tn, mr_conv2d_wgrad_tab) are RECORDED (operand pointers and geometry) instead of
 * launched; mr_tn_defer(0) stops recording.  mr_tn_flush launches everything recorded, up to mr_tn_capacity(0) = 16 problems per
 * launch, dense and conv problems together, each cut as mr_tn_group_plan says.  The 3x3 layers that mr_conv2d_wgrad_tab gives to the all-taps kernel are recorded too (their stream
 * table is still built at once): every workgroup of that kernel pays a fixed price -- prologue and a 147 KB partial tile --
 * whatever it reduced, so the flush packs up to 8 of them into one launch with fewer splits each (mr_tn_taps_plan); under
 * mr_tuning.tn_taps_fin / tn_taps_w8 / tn_splits they are launched one by one.  The caller keeps every operand alive and unmodified until the flush, flushes on the
 * stream the operands were produced on, and must not read an output (or zero it) before the flush.  mr_tn_defer returns the
 * previous setting, mr_tn_pending the number of recorded problems (both host only).  mr_tuning.tn_defer = 0 makes mr_tn_defer a
 * no-op (A/B). */
int mr_tn_defer(int on);
int mr_tn_pending(void);
/* host only: the recorded problems of one kernel; kind 0: the 128x128 TN GEMM kernel, kind 1: the all-taps kernel (mr_tn_capacity) */
int mr_tn_pending_of(int kind);
/* The queue is per DEVICE and process-wide (records pushed by one host thread are flushed by whichever thread calls mr_tn_flush
 * with that device current); mr_tn_discard drops the current device's records without launching them and switches recording off
 * for the calling thread -- for a caller whose backward pass raised and is about to release the recorded operands (round 6). */
int mr_tn_discard(void);
int mr_tn_flush(hipStream_t stream);
/* mr_tn_flush on a stream that runs CONCURRENTLY with the stream of the other weight-gradient launches (the reference leaves this
 * to cuDNN's wgrad behind nn.Conv2d / nn.LSTM backward on PyTorch's single stream, backbones/crnn.py:44-55, decoders/crnn.py:13):
 * nothing it launches touches the per-device split-reduction workspace (mr_set_tn_taps_workspace).  The caller orders the
 * stream after the producers of the recorded operands and joins it before anything reads the gradients. */
int mr_tn_flush_beside(hipStream_t stream);

/* ---- Convolution (replaces cuDNN conv fwd/dgrad/wgrad behind nn.Conv2d: backbones/crnn.py:44-55,
 *      backbones/resnet.py:39-256, backbones/ppm.py:11-44, decoders/ctc_decoder2d.py:16-27) --------------- */
int mr_conv2d_fwd(int dtype, const void* x, const void* w_krsc, const float* bias, void* y, int relu, int Nimg,
                  int H, int W, int Cin, int ldx, int Cout, int ldy, int R, int S, int sh, int sw, int ph, int pw,
                  int dh, int dw, int Ho, int Wo, hipStream_t stream);
/* conv + bias (+ ReLU) + max-pool as ONE launch (round 6): y_pool [Nimg, PHo, PWo, Cout] and the arg-max codes of mr_maxpool_fwd,
 * bit-identical to mr_conv2d_fwd followed by mr_maxpool_fwd; the full-resolution activation never reaches HBM.  bf16, stride-1
 * convolutions whose 8-wave tiles can be cut on window-row / image boundaries -- mr_conv2d_fwd_pool_ok (host only) says which;
 * replaces cuDNN conv + ReLU + MaxPool2d of backbones/crnn.py:14-33 (conv1: 2x2 / 2; conv3, conv5: 2x2, stride (2,1), pad (0,1)). */
int mr_conv2d_fwd_pool_ok(int dtype, int Nimg, int H, int W, int Cin, int ldx, int Cout, int R, int S, int sh, int sw, int ph, int pw,
                          int dh, int dw, int Ho, int Wo, int pkh, int pkw, int psh, int psw, int pph, int ppw);
int mr_conv2d_fwd_pool(int dtype, const void* x, const void* w_krsc, const float* bias, void* y_pool, unsigned char* idx, int relu,
                       int Nimg, int H, int W, int Cin, int ldx, int Cout, int R, int S, int sh, int sw, int ph, int pw, int dh,
                       int dw, int Ho, int Wo, int pkh, int pkw, int psh, int psw, int pph, int ppw, int PHo, int PWo,
                       hipStream_t stream);
/* mr_conv2d_fwd (no ReLU, ldy == Cout) that also leaves the BatchNorm batch statistics of y in bn_sums (layout and zeroing as
 * for mr_bn_stats) -- accumulated in the GEMM epilogue, so the BatchNorm that follows (reference nn.Sequential(conv, bn) at
 * backbones/resnet.py:39-56,113-181, crnn.py:48-52) skips its reduction pass over y: mr_bn_fwd_train(flags bit 3). */
int mr_conv2d_fwd_stats(int dtype, const void* x, const void* w_krsc, const float* bias, void* y, double* bn_sums, int Nimg,
                        int H, int W, int Cin, int ldx, int Cout, int R, int S, int sh, int sw, int ph, int pw, int dh,
                        int dw, int Ho, int Wo, hipStream_t stream);
/* w_crsk = weights transposed to [Cin][R][S][Cout] (mr_prep_conv_weight) */
int mr_conv2d_dgrad(int dtype, const void* dy, const void* w_crsk, void* dx, int Nimg, int H, int W, int Cin,
                    int lddx, int Cout, int lddy, int R, int S, int sh, int sw, int ph, int pw, int dh, int dw,
                    int Ho, int Wo, hipStream_t stream);
/* dx = dgrad(dy, w) + addend: the gradient of the residual branch of a ResNet block (backbones/resnet.py:152-181, `out +=
 * residual`) is added in the epilogue of the dgrad of the block's first convolution.  addend: NHWC with dx's channel count and
 * leading dimension, may alias dx, null = mr_conv2d_dgrad. */
int mr_conv2d_dgrad_add(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend, int Nimg, int H, int W,
                        int Cin, int lddx, int Cout, int lddy, int R, int S, int sh, int sw, int ph, int pw, int dh, int dw,
                        int Ho, int Wo, hipStream_t stream);
/* mr_conv2d_dgrad_add whose epilogue also accumulates the BatchNorm-BACKWARD sums of the gradient it produces: dx is the gradient
 * of y = act(bn(x) [+ residual]) of a training-mode BatchNorm (the conv -> bn -> relu chains of backbones/resnet.py:113-181);
 * bn_sums (f64 [copies][2][Cin], the scratch of mr_bn_bwd, zeroed by the caller) receives sum g' and sum g' xhat per channel
 * (g' = dx where bn_y > 0; bn_y null = no fused ReLU), and mr_bn_bwd with flags bit 3 then skips its reduction pass.  *produced
 * (host int) = 1 when the sums were written, 0 when this geometry runs on a kernel without that epilogue (dx is complete either
 * way; the caller then calls mr_bn_bwd without bit 3). */
int mr_conv2d_dgrad_bnb(int dtype, const void* dy, const void* w_crsk, void* dx, const void* addend, const void* bn_x,
                        const void* bn_y, const float* bn_mean, const float* bn_rstd, double* bn_sums, int* produced,
                        int Nimg, int H, int W, int Cin, int lddx, int Cout, int lddy, int R, int S, int sh, int sw, int ph,
                        int pw, int dh, int dw, int Ho, int Wo, hipStream_t stream);
/* dw_krsc (f32 [Cout][R][S][Cin]) and dbias (nullable, f32[Cout]) are accumulated atomically: zero them first.  Cout may be
 * smaller than lddy and need not be a multiple of the vector width when the channels Cout..lddy-1 of dy are zero padding
 * (27-channel DCN offset convolutions stored with 32): exactly Cout rows of dw / entries of dbias are written. */
int mr_conv2d_wgrad(int dtype, const void* dy, const void* x, float* dw_krsc, float* dbias, int Nimg, int H, int W,
                    int Cin, int ldx, int Cout, int lddy, int R, int S, int sh, int sw, int ph, int pw, int dh,
                    int dw, int Ho, int Wo, hipStream_t stream);
/* mr_conv2d_wgrad with a caller-owned row table of the im2col gather: rowtab = N*Ho*Wo entries of 8 bytes
 * ({element offset of the pixel's window in x, validity bit per tap}); build != 0 fills it first, build == 0 trusts
 * it (a layer's geometry is constant: build once, reuse every step).  bf16 and R*S <= 32; otherwise, or with
 * rowtab == NULL, identical to mr_conv2d_wgrad.  build bit 1: the launch may run concurrently with other weight-gradient
 * launches (another stream): the shared split-reduction workspace (mr_set_tn_taps_workspace) is not used, f32 atomics only.
 * Inside mr_tn_defer(1) the launch is recorded for mr_tn_flush (both kernels; not with build bit 1); the table is built at once. */
int mr_conv2d_wgrad_tab(int dtype, const void* dy, const void* x, float* dw_krsc, float* dbias, int N, int H, int W,
                        int Cin, int ldx, int Cout, int lddy, int R, int S, int sh, int sw, int ph, int pw, int dh,
                        int dw, int Ho, int Wo, void* rowtab, int build, hipStream_t stream);

/* ---- DB detector loss (replaces the ~100 torch launches of decoders/seg_detector_loss.py:157-185 L1BalanceCELoss =
 *      balance_cross_entropy_loss.py:29-56 + l1_loss.py:5-11 + dice_loss.py:28-42) ---------------------------------------------
 * binary / thresh / thresh_binary / gt: f32 [N, H*W] (the [N,1,H,W] maps); mask / thresh_map / thresh_mask: f32 [N, H*W].  The
 * reference multiplies gt [N,1,H,W] with mask [N,H,W]: broadcasting makes positive / negative [N,N,H,W] tensors (gt of sample a,
 * mask and loss of sample b); that is restated as is.  negloss: f32 scratch [N*N*H*W]; ws: mr_db_loss_ws_bytes() bytes ZEROED by
 * the caller; out: f32 [16] = {loss, bce, l1, dice, state read by mr_db_loss_bwd ...}.  The sum of the nc largest negative losses
 * is an exact radix selection; elements tied at the threshold share the remaining count equally in the gradient. */
long long mr_db_loss_ws_bytes(void);
/* tail of the two DB heads (decoders/seg_detector.py:77-79,142-147): binary = sigmoid(xb), thresh = sigmoid(xt) -- float32 outputs
 * whatever `dtype` the logits have -- and thresh_binary = 1 / (1 + exp(-k (binary - thresh))); n elements each */
int mr_db_head_tail_fwd(int dtype, const void* xb, const void* xt, float* binary, float* thresh, float* tbinary, long long n,
                        float k, hipStream_t stream);
int mr_db_head_tail_bwd(int dtype, const float* binary, const float* thresh, const float* tbinary, const float* gb,
                        const float* gt, const float* gtb, void* dxb, void* dxt, long long n, float k, hipStream_t stream);
int mr_db_loss_fwd(const float* binary, const float* thresh, const float* tbinary, const float* gt, const float* mask,
                   const float* tmap, const float* tmask, float* negloss, void* ws, float* out, int N, long long HW,
                   float negative_ratio, float eps, float l1_scale, float bce_scale, hipStream_t stream);
int mr_db_loss_bwd(const float* binary, const float* thresh, const float* tbinary, const float* gt, const float* mask,
                   const float* tmap, const float* tmask, const float* out, const float* gloss, float* g_binary,
                   float* g_thresh, float* g_tbinary, int N, long long HW, float l1_scale, float bce_scale,
                   hipStream_t stream);

/* ---- layout / elementwise helpers ---------------------------------------------------------------------- */
int mr_nchw_to_nhwc(int dtype, const float* src, void* dst, int N, int C, int H, int W, int Cpad,
                    hipStream_t stream);
int mr_nhwc_to_nchw(int dtype, const void* src, float* dst, int N, int C, int H, int W, int ld, hipStream_t stream);
int mr_cast(int src_dtype, const void* src, int dst_dtype, void* dst, long long n, hipStream_t stream);
int mr_relu_bwd(int dtype, const void* dy, const void* y, void* dx, long long n, hipStream_t stream);
int mr_add(int dtype, const void* a, const void* b, void* out, long long n, int relu, hipStream_t stream);
/* out[perm(c)] (f32) += sum_p x[p,c] */
int mr_colsum(int dtype, const void* x, float* out, int P, int C, long long ld, int perm_h, hipStream_t stream);
/* [A,B,C] -> [B,A,C] */
int mr_permute_021(int dtype, const void* src, void* dst, int A, int B, int C, hipStream_t stream);
/* fp32 master weights (logical [K][C][R][S], arbitrary strides) -> operand images of `dtype`:
 * dst_krsc [K][R][S][Cpad] (zero padded channels), dst_crsk [C][R][S][ldk] (transposed, for dgrad); either may be null */
int mr_prep_conv_weight(int dtype, const float* src, long long sk, long long sc, long long sr, long long ss,
                        void* dst_krsc, void* dst_crsk, int K, int C, int R, int S, int Cpad, int ldk,
                        hipStream_t stream);
/* src f32 [R][C] with row stride lds (elements) -> dst_n [R][ldn] and/or dst_t [C][ldt] of `dtype` (rows permuted to
 * the gate-interleaved order when perm_h > 0) */
int mr_prep_matrix(int dtype, const float* src, int lds, void* dst_n, int ldn, void* dst_t, int ldt, int R, int C,
                   int perm_h, hipStream_t stream);
int mr_prep_bias(const float* a, const float* b, float* dst, int R, int perm_h, hipStream_t stream);

/* All of the above in ONE launch.  The host keeps a table of prep jobs in device memory (it only changes when the
 * set of parameters changes) and re-runs it after every optimizer update -- the fp32 master -> compute-dtype operand
 * images of every layer are regenerated together instead of by ~3 small kernels per layer per step.
 *   MR_PREP_CONV:   mr_prep_conv_weight(src, s0..s3 = sk,sc,sr,ss, dst_a = krsc, dst_b = crsk, d0..d3 = K,C,R,S,
 *                   pad = Cpad, ld_b = ldk)
 *   MR_PREP_MATRIX: mr_prep_matrix(src, s0 = lds, dst_a = dst_n, pad = ldn, dst_b = dst_t, ld_b = ldt, d0,d1 = R,C,
 *                   perm_h)
 *   MR_PREP_BIAS:   mr_prep_bias(src, src2, dst_a (f32), d0 = R, perm_h)
 *   MR_PREP_STEM:   mr_stem_pack(src, s0..s3 = sk,sc,sr,ss, dst_a = wpack, d1 = Cin)   (one block)
 * Work unit = one 64x64 tile of the job's logical matrix (conv: K rows x R*S*Cpad columns; matrix: R x C; bias:
 * 4096 elements).  The jobs are laid end to end on the grid: job.block_start = index of its first tile (jobs
 * sorted by block_start, job 0 starts at 0); total_blocks = sum over jobs of
 *   conv: ceil(K/64)*ceil(R*S*Cpad/64), matrix: ceil(R/64)*ceil(C/64), bias: ceil(R/4096), stem: 1.
 * Transposed images need dst_b 16-byte aligned and ld_b a multiple of one 16-byte vector for the fast path. */
#define MR_PREP_CONV 0
#define MR_PREP_MATRIX 1
#define MR_PREP_BIAS 2
#define MR_PREP_STEM 3
typedef struct mr_prep_job {
  const float* src;
  const float* src2;
  void* dst_a;
  void* dst_b;
  long long s0, s1, s2, s3;
  int kind;
  int d0, d1, d2, d3;
  int pad, ld_b, perm_h;
  int block_start, reserved;
} mr_prep_job;
int mr_prep_batch(int dtype, const mr_prep_job* jobs_device, int njobs, long long total_blocks, float* tick,
                  hipStream_t stream);   /* tick (nullable): an optimizer's hyper block whose step counter this launch advances */
/* sizeof(mr_prep_job) as compiled into the library (host only): bindings verify their struct mirror against it */
int mr_sizeof_prep_job(void);

/* dst[i][0..n[i]) += src[i][0..n[i]) for count <= MR_MAX_SEGMENTS f32 segments in one launch (the pointer / length
 * arrays are HOST arrays, copied into the kernel arguments).  Used to fold several small gradient pieces into the
 * optimizer's flat gradient buffer (replaces one `grad += piece` kernel per parameter). */
#define MR_MAX_SEGMENTS 8
int mr_accumulate_multi(int count, float* const* dst, const float* const* src, const long long* n,
                        hipStream_t stream);
/* zero fill of count <= MR_MAX_SEGMENTS buffers (16-byte aligned, sizes multiples of 16 bytes) in one launch: zero_grad() of the
 * fused optimizers clears the flat gradient buffers and the pre-zeroed scratch arena together */
int mr_zero_multi(int count, void* const* dst, const long long* bytes, hipStream_t stream);

/* ---- optimizers (replaces torch.optim.Adam / SGD at training/optimizer_scheduler.py:17-22) -------------- */
/* hyper: device f32[8] = {lr, beta1 (SGD: momentum), beta2, eps, weight_decay, completed steps, gradient scale (0 = 1), -}.
 * The update kernels run step hyper[5] + 1 and only READ the counter; the launch behind them advances it: mr_prep_batch(tick =
 * hyper) -- the regeneration of the weight images that follows every update anyway -- or mr_opt_tick.  hipGraph-replay safe. */
int mr_opt_tick(float* hyper, hipStream_t stream);
int mr_adam_step(float* p, const float* g, float* m, float* v, long long n, float* hyper, hipStream_t stream);
int mr_sgd_step(float* p, const float* g, float* buf, long long n, float* hyper, hipStream_t stream);

/* ---- BatchNorm2d / MaxPool2d (backbones/crnn.py:17-31,49-52; backbones/resnet.py:26-30,199) ------------- */
/* doubles of reduction scratch mr_bn_fwd_train / mr_bn_bwd want for C channels: 8 accumulator copies of [2][C] (fewer
 * same-address atomics) followed by C doubles the backward uses -- the unfused path for 2*C f32 per-channel means, the one-pass
 * path (mr_tuning.bn_onepass) for one arrival counter per 64-channel slab, 512 bytes apart.  "Zeroed" below means the WHOLE
 * scratch. */
long long mr_bn_scratch_doubles(int C);
/* training-mode BN folds its finalize kernels into the apply passes (C % 64 == 0) unless mr_tuning.bn_fused = 0 */
int mr_bn_fwd_train(int dtype, const void* x, void* y, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float* save_mean, float* save_rstd, double* sums, const void* residual,
                    int relu, long long P, int C, float eps, float momentum, long long* num_batches_tracked,
                    hipStream_t stream); /* num_batches_tracked (nullable): int64 step counter, incremented by one;
                                          relu: bit0 fused ReLU, bit2 `sums` is already zero (skip the memset), bit3 `sums`
                                          already HOLDS the statistics (mr_conv2d_fwd_stats / mr_bn_stats): no reduction pass */
/* the statistics pass on its own: sums (f64 [8][2][C] = the first 16*C doubles of the mr_bn_scratch_doubles(C) scratch, zeroed by
 * the caller) += per-channel sum / sum of squares of x [P][C] */
int mr_bn_stats(int dtype, const void* x, double* sums, long long P, int C, hipStream_t stream);
int mr_bn_fwd_eval(int dtype, const void* x, void* y, const float* gamma, const float* beta,
                   const float* running_mean, const float* running_var, float* tmp_mean, float* tmp_rstd,
                   const void* residual, int relu, long long P, int C, float eps, hipStream_t stream);
int mr_bn_bwd(int dtype, const void* dy, const void* x, const void* y, const float* gamma, const float* save_mean,
              const float* save_rstd, double* sums, void* dx, void* dres, float* dgamma, float* dbeta, int flags,
              long long P, int C, hipStream_t stream); /* flags: bit0 fused ReLU, bit1 accumulate into dgamma/dbeta, bit2 `sums`
                                          is already zero (all mr_bn_scratch_doubles(C) of it), bit3 `sums` already holds the two
                                          reductions (mr_conv2d_dgrad_bnb).  Tensors that fit one resident grid (C % 64 == 0,
                                          P * C * sizeof(T) < 2 GiB) take ONE launch with a barrier among the workgroups of a
                                          64-channel slab (bounded wait; a workgroup that times out poisons its outputs with NaN);
                                          the others the reduction launch + the apply launch. */
int mr_maxpool_fwd(int dtype, const void* x, void* y, unsigned char* idx, int N, int H, int W, int C, int kh,
                   int kw, int sh, int sw, int ph, int pw, int Ho, int Wo, hipStream_t stream);
/* relu_y (nullable): the pool's OUTPUT [N,Ho,Wo,C] when its input is the output of a ReLU -- fuses that ReLU's backward
 * mask (value at the arg-max position == pooled output, so the mask is read at pooled resolution) */
int mr_maxpool_bwd(int dtype, const void* dy, const unsigned char* idx, const void* relu_y, void* dx, int N, int H,
                   int W, int C, int kh, int kw, int sh, int sw, int ph, int pw, int Ho, int Wo,
                   hipStream_t stream);

/* ---- fused backbone stem: Conv2d(Cin -> 64, 3x3, s1, p1) + bias + ReLU + MaxPool2d(2,2) -----------------------
 * replaces cnn.conv0 / relu0 / pooling0 of reference backbones/crnn.py:17-19,48-55 in one pass each way.
 * x: fp32 NCHW contiguous [N,Cin,H,W] (Cin 1 or 3, even H and W); w: fp32 [64,Cin,3,3] with element strides
 * wsk,wsc,wsr,wss; y: pooled activation NHWC [N,H/2,W/2,64] of `dtype`; code: one byte per pooled element
 * (bits 0-1 = first-maximum position in the 2x2 window, bit 2 = maximum > 0).  code == NULL in mr_stem_fwd means
 * "do not write the codes" (inference: only mr_stem_bwd reads them); y is the same either way.
 * mr_stem_bwd ACCUMULATES into dw (strides dsk..dss) and dbias (either may be null); workspace must hold
 * mr_stem_bwd_workspace(Cin) floats and need not be initialised (every float that is read was written by the same
 * call).  The layer's input gradient is not produced (the input is the image). */
long long mr_stem_bwd_workspace(int Cin);
/* wpack (bf16 [64][32], k = (dr*3+ds)*Cin + c, zero padded): the filter bank pre-packed for the bf16 MFMA kernel by
 * mr_stem_pack / an MR_PREP_STEM job.  When it is null (or dtype is f32, or W/2 is not a multiple of 16) mr_stem_fwd
 * runs the generic FMA kernel straight from w.  The MFMA kernels read x with 16-byte loads when x is 16-byte aligned
 * (dword loads otherwise); mr_stem_bwd takes its MFMA path only when dy is 8-byte and code 4-byte aligned. */
int mr_stem_pack(const float* w, long long wsk, long long wsc, long long wsr, long long wss, void* wpack, int Cin,
                 hipStream_t stream);
int mr_stem_fwd(int dtype, const float* x, const float* w, long long wsk, long long wsc, long long wsr,
                long long wss, const void* wpack, const float* bias, void* y, unsigned char* code, int N, int Cin,
                int H, int W, hipStream_t stream);
int mr_stem_bwd(int dtype, const void* dy, const unsigned char* code, const float* x, float* workspace, float* dw,
                long long dsk, long long dsc, long long dsr, long long dss, float* dbias, int N, int Cin, int H,
                int W, hipStream_t stream);

/* ---- bidirectional LSTM recurrence (replaces cuDNN RNN behind nn.LSTM: decoders/crnn.py:13,21,91-93) ----- */
/* ws / ws_bytes: exchange workspace of the persistent one-launch recurrence (size from mr_lstm_ws_bytes; zeroed by
 * the call with a memset on `stream`; its last 256 bytes hold a status word: 0 = ok, 1 / 2 = a bounded spin of the
 * forward / backward kernel timed out).  Null / 0 selects one launch per time step.  dc is only used by the
 * per-step path (f32 [N, 2H] scratch). */
int mr_lstm_fwd(int dtype, const void* xproj, const void* whh, void* out, float* cbuf, void* gates, int T, int N,
                int H, void* ws, long long ws_bytes, hipStream_t stream);
int mr_lstm_bwd(int dtype, const void* dout, const void* whhT, const float* cbuf, void* gates, float* dc, int T,
                int N, int H, void* ws, long long ws_bytes, hipStream_t stream);
/* host only: workspace bytes the persistent recurrence wants (0 = not applicable: f32, H != 256, mr_tuning.lstm_persist = 0) */
long long mr_lstm_ws_bytes(int dtype, int T, int N, int H);
/* debug hook (host only): non-null -> the persistent backward also writes its reduced recurrent term [T,N,2H] f32 */
int mr_lstm_debug_buffer(float* p);
/* (column-tile width of the step kernels: mr_tuning.lstm_fwd_bn / lstm_bwd_bn; 0 = LDS-staged split-K body, else the
 * direct-fragment body) */

/* ---- 1-D CTC fused with log-softmax (replaces log_softmax + nn.CTCLoss: decoders/crnn.py:48,96-98) ------- */
int mr_ctc_fwd(int dtype, const void* logits, int ldl, const void* targets, int targets_i64,
               const void* input_lengths, const void* target_lengths, int lengths_i64, int T, int N, int C, int S,
               int blank, int zero_infinity, float* log_probs, double* alpha, double* beta, double* nll,
               double* loss, double* log_probs_f64, hipStream_t stream);
/* log_probs_f64 (nullable, f64 [T][N][C]): the same log-probabilities widened to float64 -- what the reference returns as
 * `pred` (decoders/crnn.py:96 `log_softmax(pred, dim=2).to(torch.float64)`), written by the same kernel.
 * mr_ctc_bwd writes every element of grad_logits [T][N][ldg] exactly once, the padding columns C .. ldg-1 as zeros.
 * C is not limited.  Up to the alphabet whose four float rows fit in 64 KB of LDS next to the 2S+1 states (S = 32: C <= 3 932) the
 * per-sample kernels do the log-softmax themselves and the gradient kernel stages its rows in LDS; beyond it (mr_ctc_wide) a
 * row-parallel log-softmax over all T*N rows runs in front of the recursions and the gradient kernel streams the classes from HBM,
 * with nothing per class in LDS.  S is limited by the LDS of the recursion: (2S+1) * 36 + 16 <= 64 KB.
 * alpha, beta: f64 [N][T][2S+1] -- scratch that travels from mr_ctc_fwd to mr_ctc_bwd: the log-domain forward / backward
 * variables (mr_tuning.ctc_linear = 0, or an emission table beyond 64 KB of LDS) or, by default, their scaled linear-domain
 * counterparts (alpha rescaled per step by exact powers of two; beta without the emission of its own step).  beta may be null in mr_ctc_fwd when no gradient is wanted (the beta recursion runs
 * concurrently with alpha on other wavefronts of the same workgroup, so storing it costs no extra latency and makes
 * the gradient kernel independent per (t, n) row). */
int mr_ctc_bwd(int dtype, const float* log_probs, const double* alpha, const double* beta, const double* nll,
               const void* targets, int targets_i64, const void* input_lengths, const void* target_lengths,
               int lengths_i64, const double* grad_out, int T, int N, int C, int S, int blank, int zero_infinity,
               void* grad_logits, int ldg, hipStream_t stream);
/* host only: 1 when mr_ctc_fwd / mr_ctc_bwd serve an alphabet of C classes and targets padded to S with the wide kernels */
int mr_ctc_wide(int C, int S);

/* ---- 2D-CTC (replaces the CUDA extension ops/ctc_2d: csrc/ctc2d.h:7-43, cuda/ctc2d_cuda_kernel.cu) -------------
 * log_probs [T,H,N,C] contiguous (`dtype`), targets [N,S] i64, lengths [N] i64.  Reference pybind signatures:
 *   ctc2d_forward(log_probs, targets, input_lengths, target_lengths, BLANK, TINY) -> (nll[N], log_alpha[N,T,H,2S+1])
 *   ctc2d_backward(grad_out, log_probs, targets, input_lengths, target_lengths, nll, log_alpha, BLANK) -> grad
 * Here the caller allocates nll / alpha (f32), the beta scratch (f32, same shape as alpha) and grad (`dtype`). */
int mr_ctc2d_fwd(int dtype, const void* log_probs, const long long* targets, const long long* input_lengths,
                 const long long* target_lengths, int T, int H, int N, int C, int S, int blank, float* nll,
                 float* alpha, hipStream_t stream);
int mr_ctc2d_bwd(int dtype, const float* grad_out, const void* log_probs, const long long* targets,
                 const long long* input_lengths, const long long* target_lengths, const float* nll,
                 const float* alpha, float* beta, void* grad, int T, int H, int N, int C, int S, int blank,
                 hipStream_t stream);

/* ---- ResNet50-dilated / PPM / 2D-CTC head helpers (backbones/ppm.py:11-44, decoders/ctc_decoder2d.py:16-45) ----- */
int mr_adaptive_avgpool_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, int OH, int OW,
                            hipStream_t stream);
int mr_adaptive_avgpool_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int C, int OH, int OW,
                            hipStream_t stream);
/* Pyramid pooling (reference backbones/ppm.py:13-20,36-40): nscales (<= 8) adaptive average pools of ONE map per launch.  ys / dys:
 * host arrays of device pointers [N][oh[i]][ow[i]][C].  Forward outputs are bit-identical to mr_adaptive_avgpool_fwd's; backward
 * writes dx = sum_i adaptive_avgpool_bwd(dys[i]) (f32 accumulation, one rounding).  H * W * 128 bytes must fit 64 KB of LDS. */
int mr_adaptive_avgpool_multi_fwd(int dtype, const void* x, void* const* ys, const int* oh, const int* ow, int nscales, int N,
                                  int H, int W, int C, hipStream_t stream);
int mr_adaptive_avgpool_multi_bwd(int dtype, void* const* dys, const int* oh, const int* ow, int nscales, void* dx, int N, int H,
                                  int W, int C, hipStream_t stream);
/* bilinear resize, align_corners=False; writes channels [coff, coff+C) of rows with stride ldy; accumulate=1 adds */
int mr_bilinear_fwd(int dtype, const void* x, void* y, int N, int H, int W, int C, int OH, int OW, int ldy, int coff,
                    int accumulate, hipStream_t stream);
int mr_bilinear_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int C, int OH, int OW, int lddy,
                    int coff, hipStream_t stream);
/* nearest-neighbour upsampling by an integer factor s (decoders/seg_detector.py:22-43): y[n,oh,ow,coff+c] =
 * x[n,oh/s,ow/s,c] (+ add[n,oh,ow,c], nullable); backward sums the s x s block */
int mr_nearest_up_fwd(int dtype, const void* x, const void* add, void* y, int N, int H, int W, int C, int s, int ldy,
                      int coff, hipStream_t stream);
int mr_nearest_up_bwd(int dtype, const void* dy, void* dx, int N, int H, int W, int C, int s, int lddy, int coff,
                      hipStream_t stream);
/* nn.ConvTranspose2d(cin, cout, 2, 2) of the DB heads (decoders/seg_detector.py:66-79) = a GEMM y2[p, co*4 + i*2 + j] = sum_ci
 * x[p, ci] W[ci, co, i, j] (mr_gemm_nt on the weight's own [Cin][Cout*4] matrix) + this depth-to-space pass with the bias:
 * y[n, 2h+i, 2w+j, co] = y2[p, (co, i, j)] + bias[co].  y2 [N*H*W][ld2 >= 4*C], y NHWC [N, 2H, 2W, C], bias f32 nullable. */
int mr_deconv2x2_d2s(int dtype, const void* y2, int ld2, const float* bias, void* y, int N, int H, int W, int C,
                     hipStream_t stream);
/* the inverse gather for backward: dy2[p, (co, i, j)] = dy[n, 2h+i, 2w+j, co], columns 4*C .. ld2-1 zero */
int mr_deconv2x2_s2d(int dtype, const void* dy, void* dy2, int ld2, int N, int H, int W, int C, hipStream_t stream);
int mr_copy_channels(int dtype, const void* src, int lds, int soff, void* dst, int ldd, int doff, long long P, int C,
                     hipStream_t stream);
/* dx [N, H, W, C] <- the gradient of the sub-sampling x[:, ::sh, ::sw, :]: dxs [N, Ho, Wo, C] at the sampled positions, zeros
 * elsewhere (one pass over dx).  With mr_conv2d_dgrad on the sub-sampled grid this is the data gradient of a strided 1x1
 * convolution without padding (the downsample branch of a ResNet stage, backbones/resnet.py:204-213). */
int mr_scatter_strided(int dtype, const void* dxs, void* dx, int N, int H, int W, int C, int sh, int sw, int Ho, int Wo,
                       hipStream_t stream);
int mr_scale_channels(int dtype, const void* x, const float* scale, void* y, int N, long long HW, int C,
                      hipStream_t stream);
/* lp[w,h,n,c] = log(max(softmax_h(mask)[n,h,w] * softmax_c(cls)[n,h,w,c], tiny)); also returns both softmaxes (f32) */
int mr_ctc2d_head_fwd(int dtype, const void* mask_logits, int lda, const void* cls_logits, int ldz, float* lp,
                      float* mask_prob, float* cls_prob, int N, int H, int W, int C, float tiny, hipStream_t stream);
int mr_ctc2d_head_bwd(int dtype, const float* grad_lp, const float* mask_prob, const float* cls_prob, void* dmask,
                      int ldda, void* dcls, int lddz, int N, int H, int W, int C, float tiny, hipStream_t stream);

/* ---- Modulated deformable conv v2 (replaces assets/ops/dcn: src/deform_conv_cuda.cpp:486-679 and
 *      src/deform_conv_cuda_kernel.cu:569-766; python API functions/deform_conv.py:108-177) --------------------------
 * Fused path (csrc/dcn_fused.hip; C % 64 == 0, Co % 64 == 0, kh*kw <= 9 -- every DCN layer of deformable_resnet50): the column
 *   matrix never exists.  forward = sample -> LDS -> MFMA; backward = offset / mask gradients from gcol tiles kept in the MFMA
 *   accumulators, input gradient as a CSR-inverted GATHER-GEMM (no f32 atomics), dW / dbias by a TN GEMM whose operand is
 *   sampled on the fly.
 * General path (any C % vector == 0): the three piecewise kernels below around mr_gemm_nt / mr_gemm_tn:
 *   forward  = mr_dcn2_im2col (whole batch) + mr_gemm_nt(col, w_krsc, bias)
 *   backward = mr_gemm_nt(dy, w^T) -> gcol; mr_dcn2_coord_grad; mr_dcn2_col2im; mr_dcn2_im2col + mr_gemm_tn (dW, dbias)
 * offset / mask are f32 and indexed per sample as FLAT [2*kh*kw][Ho][Wo] / [kh*kw][Ho][Wo] arrays from the sample's
 * base (per-sample strides off_bs / msk_bs), exactly like deform_conv_cuda_kernel.cu:599-612. */
int mr_dcn2_im2col(int dtype, const void* x, const float* offset, long long off_bs, const float* mask,
                   long long msk_bs, void* col, int N, int H, int W, int C, int kh, int kw, int stride, int pad,
                   int dil, int Ho, int Wo, hipStream_t stream);
int mr_dcn2_coord_grad(int dtype, const void* gcol, const void* x, const float* offset, long long off_bs,
                       const float* mask, long long msk_bs, float* doffset, float* dmask, int N, int H, int W,
                       int C, int kh, int kw, int stride, int pad, int dil, int Ho, int Wo, hipStream_t stream);
int mr_dcn2_col2im(int dtype, const void* gcol, const float* offset, long long off_bs, const float* mask,
                   long long msk_bs, float* dx, int N, int H, int W, int C, int kh, int kw, int stride, int pad,
                   int dil, int Ho, int Wo, hipStream_t stream);

/* single-call forms (replace modulated_deform_conv_cuda_forward / _backward,
 * assets/ops/dcn/src/deform_conv_cuda.cpp:486-679).  Caller owns all buffers incl. the workspace col_ws (the reference passes
 * `columns` the same way, functions/deform_conv.py:135) of mr_dcn2_ws_bytes(..., backward) bytes -- 0 for the fused forward
 * (col_ws may be NULL), the CSR of the scatter pattern for the fused backward, the column matrix [N*Ho*Wo, kh*kw*C] otherwise.
 * w_n [Co][kh*kw*C] / w_t [kh*kw*C][Co] are the mr_prep_matrix images of the KRSC weight; dx32 / doffset / dmask are ACCUMULATED
 * into and must arrive zeroed (the reference's Function allocates them with zeros_like, functions/deform_conv.py:150-154);
 * dw f32 [Co][kh*kw*C] and dbias f32 [Co] accumulated.  Any of the three output groups -- {doffset, dmask}, dx32, {dw, dbias} --
 * may be null: only the others are computed. */
long long mr_dcn2_ws_bytes(int dtype, int N, int H, int W, int C, int Co, int kh, int kw, int Ho, int Wo, int backward);
/* (mr_tuning.dcn_fused = 0: general kernels for every shape; mr_tuning.dcn_v1_bwd: backward variant of the general path) */
int mr_dcn2_fwd(int dtype, const void* x, const void* w_n, const float* bias, const float* offset, long long off_bs,
                const float* mask, long long msk_bs, void* y, void* col_ws, int N, int H, int W, int C, int Co, int kh,
                int kw, int stride, int pad, int dil, int Ho, int Wo, hipStream_t stream);
int mr_dcn2_bwd(int dtype, const void* dy, const void* x, const void* w_t, const float* offset, long long off_bs,
                const float* mask, long long msk_bs, void* col_ws, float* dx32, float* doffset, float* dmask, float* dw,
                float* dbias, int N, int H, int W, int C, int Co, int kh, int kw, int stride, int pad, int dil, int Ho,
                int Wo, hipStream_t stream);
/* host only: 1 when the fused kernels serve this shape (C and Co multiples of 64, at most 9 taps, mr_tuning.dcn_fused) */
int mr_dcn2_fused(int dtype, int H, int W, int C, int Co, int kh, int kw);
/* host only: 1 when mr_dcn2_bwd2 can write the input gradient in `dtype` directly (dx_t) for this shape */
int mr_dcn2_dx_direct(int dtype, int N, int H, int W, int C, int Co, int kh, int kw);
/* mr_dcn2_bwd with: dx_t (nullable, INSTEAD of dx32) = the input gradient in `dtype`, overwritten (no zero fill, no conversion
 * pass; only where mr_dcn2_dx_direct says 1); flags bit 0 = col_ws was zeroed once and has been used by this function only
 * since (its counters clean themselves): the memset node in front of the CSR build is dropped. */
int mr_dcn2_bwd2(int dtype, const void* dy, const void* x, const void* w_t, const float* offset, long long off_bs,
                 const float* mask, long long msk_bs, void* col_ws, float* dx32, void* dx_t, int flags, float* doffset,
                 float* dmask, float* dw, float* dbias, int N, int H, int W, int C, int Co, int kh, int kw, int stride, int pad,
                 int dil, int Ho, int Wo, hipStream_t stream);
/* round 6: mr_dcn2_col_saved (host only) = 1 when mr_dcn2_fwd leaves the sampled column matrix [N*Ho*Wo, kh*kw*C] in its col_ws
 * (bf16, mr_tuning.dcn_col_fwd); mr_dcn2_bwd3 = mr_dcn2_bwd2 + col_saved (nullable): that buffer, kept alive by the caller --
 * the weight gradient reads it instead of sampling x again. */
int mr_dcn2_col_saved(int dtype, int H, int W, int C, int Co, int kh, int kw);
int mr_dcn2_bwd3(int dtype, const void* dy, const void* x, const void* w_t, const float* offset, long long off_bs,
                 const float* mask, long long msk_bs, void* col_ws, float* dx32, void* dx_t, int flags, float* doffset,
                 float* dmask, float* dw, float* dbias, const void* col_saved, int N, int H, int W, int C, int Co, int kh, int kw,
                 int stride, int pad, int dil, int Ho, int Wo, hipStream_t stream);
/* Packed offset/mask operand of the deformable ResNet blocks (reference backbones/resnet.py:125-142: offset_mask =
 * conv2_offset(x); conv2(x, offset_mask[:, :18], offset_mask[:, -9:].sigmoid())).  raw = the offset conv's output, NHWC
 * [N][HW][ld] in `dtype` (channels n_offset + n_mask <= ld).  mr_dcn_unpack writes the flat f32 NCHW offset [N][n_offset][HW]
 * and mask = sigmoid(logits) [N][n_mask][HW] that mr_dcn2_fwd / _bwd read; mr_dcn_pack_grad folds their gradients back into
 * d raw (dmask * m * (1 - m) for the mask logits, zeros in the padding channels).  One launch each: they replace the slice,
 * cast, contiguous, sigmoid, sigmoid_backward, slice_backward and add launches of the unfused autograd graph. */
int mr_dcn_unpack(int dtype, const void* raw, int ld, float* offset, float* mask, int N, int HW, int n_offset, int n_mask,
                  hipStream_t stream);
int mr_dcn_pack_grad(int dtype, const float* doffset, const float* dmask, const float* mask, void* graw, int ld, int N,
                     int HW, int n_offset, int n_mask, hipStream_t stream);

/* ---- Deformable PS-RoI pooling (assets/ops/dcn/src/deform_pool_cuda.cpp:30-77 deform_psroi_pooling_cuda_forward /
 * _backward; kernels deform_pool_cuda_kernel.cu:52-143, 146-268).  data [B][C][H][W] f32, rois [R][5] (batch index, x1,
 * y1, x2, y2), trans [R][channels_trans][part][part] (ignored when no_trans), out / top_count / out_grad
 * [R][output_dim][P][P]; all caller-allocated.  bwd ACCUMULATES into data_diff / trans_diff (caller zero-fills, as
 * functions/deform_pool.py:57-59 does). */
int mr_deform_psroi_fwd(const float* data, const float* rois, const float* trans, float* out, float* top_count, int B,
                        int C, int H, int W, int R, int channels_trans, int no_trans, float spatial_scale,
                        int output_dim, int group_size, int pooled_size, int part_size, int sample_per_part,
                        float trans_std, hipStream_t stream);
int mr_deform_psroi_bwd(const float* out_grad, const float* data, const float* rois, const float* trans,
                        const float* top_count, float* data_diff, float* trans_diff, int B, int C, int H, int W, int R,
                        int channels_trans, int no_trans, float spatial_scale, int output_dim, int group_size,
                        int pooled_size, int part_size, int sample_per_part, float trans_std, hipStream_t stream);

/* ---- DB detector post-processing (structure/representers/seg_detector_representer.py:63-168): the per-pixel stages.
 * mr_db_components: prob f32 [N][H][W] thresholded (> thresh) -> labels i32 [N][H][W] (root pixel index of the
 * 8-connected component, -1 background) and the run end points of every component, points int4 [cap] = (n, root, x, y),
 * *count = their number (zero on entry; may exceed cap).  mr_db_box_scores: boxes f32 [B][9] = image index + 4 vertices
 * in order; out f32 [B][2] = (sum of prob, pixel count) over the pixels inside or on the border of each box. */
int mr_db_components(const float* prob, float thresh, int* labels, void* points, int* count, int cap, int N, int H, int W,
                     hipStream_t stream);
int mr_db_box_scores(const float* prob, const float* boxes, float* out, int B, int N, int H, int W, hipStream_t stream);
/* mr_db_boxes: the whole of `boxes_from_bitmap` for a batch on the device, no host synchronisation; float64 geometry that restates
 * megreader_amd/structure/db_geometry.py operation for operation (math.hypot of non-integers as sqrt(x*x + y*y)); integer atomics
 * only, the same bits every run.  prob f32 [N][H][W] is scored, seg f32 [N][H][W] is thresholded (> thresh) into regions (may be
 * prob); dest i32 [N][2] = (width, height) the boxes of image n are scaled to.  Candidate k of image n = its k-th 8-connected
 * component in raster order of its first pixel, k < K; components i32 [N] = how many the image has (> K: truncated).
 * Per candidate: `mini_box` of its pixels, dropped when the short side < min_size; score = sum / count of prob over the
 * truncated box (the arithmetic of mr_db_box_scores), dropped when box_thresh > score; `unclip` and `mini_box` again, dropped
 * when the short side < min_size + 2; corners scaled by dest / (W, H), rounded half-even, clamped to [0, dest].
 * boxes f64 [N][K][4][2] / scores f32 [N][K]: the surviving boxes in candidate order, count i32 [N] of them, zeros behind.
 * Optional (NULL = not wanted), per candidate slot: cand f64 [N][K][4][2] the ordered rectangle before unclip, cand_sums
 * f32 [N][K][2] its (sum, count) (zeros when not scored), status i32 [N][K]: 0 no such component, 1 short side < min_size,
 * 2 below box_thresh, 3 too small after unclip, 4 kept.
 * ws: *bytes of mr_db_boxes_ws_bytes (labels, rank map, row counts, the table of row extremes i32 [N][K][H][2], uncompacted
 * results, the candidate rectangles f64 [N][K][4][2] that mr_db_ribbons reads), 16-byte aligned, not initialised.  1 <= K <= 1024; H <= 2048 (a candidate's 2 H hull points are staged in LDS);
 * H * W < 2^31; MR_ERR_ARG otherwise. */
int mr_db_boxes_ws_bytes(int N, int H, int W, int K, long long* bytes);
int mr_db_boxes(const float* prob, const float* seg, float thresh, const int* dest, int N, int H, int W, int K,
                double box_thresh, double min_size, void* ws, double* boxes, float* scores, int* count, int* components,
                double* cand, float* cand_sums, int* status, hipStream_t stream);
/* mr_db_ribbons: a RIBBON beside every box of the preceding mr_db_boxes, for words that follow a curve.  A ribbon is k rulings, each
 * a top point and a bottom point in dest coordinates, ordered along the reading direction; the word is the strip between the two
 * polylines (mr_strip_crop rectifies it).  Called after mr_db_boxes on the same stream with the same N, H, W, K, dest and ws: it
 * reads what that call left there (flattened labels, row extremes, statuses and candidate rectangles), one launch, no host
 * synchronisation, capturable; float64 with every product and sum rounded on its own, integer atomics only, the same bits every
 * run (tests/_db_ribbon_ref.py restates it).  For the j-th surviving box of image n (the order of `boxes`):
 *   ribbons f64 [N][K][MR_RIBBON_MAX_KNOTS][2][2] (knot, top / bottom, x / y), zeros behind the used knots;
 *   knots i32 [N][K]: 0 = no ribbon, the box stands; otherwise 5 .. MR_RIBBON_MAX_KNOTS;
 *   why i32 [N][K]: 0 ribbon, 1 short, 2 empty slab, 3 steep, 4 folded.     Rows behind count[n]: zeros.
 *   rws: *bytes of mr_db_ribbons_ws_bytes, 8-byte aligned, not initialised: i64 [N][K][MR_RIBBON_MAX_SLABS][6], per candidate SLOT
 *   with a kept box that reached step 3 the sums of its Se slabs (the rest is not written).
 * The rule, per candidate whose status is kept; p0..p3 = its ordered rectangle before unclip (`cand`), |v| = sqrt(v.x*v.x + v.y*v.y),
 * S = slabs, expressions evaluated left to right:
 *  1. axis   a = |p1 - p0|, b = |p3 - p0|.  max((int)b, 1) > 1.5 * max((int)a, 1):  o = p1, e = (p2 - p1) / b, L = b;  otherwise
 *            o = p0, e = (p1 - p0) / a, L = a  (`plan_crop`'s `rotated` rule: a vertical word reads downwards).  L > 0, else short.
 *  2. slabs  P = pixels of the component, tbar = P / (L + 1), Se = min(S, (int)((L + 1) / max(4.0, tbar))); Se < 3: short.
 *            sw = (L + 1) / Se; pixel (x, y) lies in slab clamp((int)floor((u + 0.5) / sw), 0, Se - 1), u = (x - o.x)*e.x + (y - o.y)*e.y.
 *  3. moments per slab, 64-bit integers: n, Sx, Sy, Sxx, Sxy, Syy.  Any n == 0: empty.  m = (Sx / n, Sy / n),
 *            cxx = Sxx / n - m.x*m.x, cxy = Sxy / n - m.x*m.y, cyy = Syy / n - m.y*m.y.
 *  4. tangents  t_j = m_{j+1} - m_{j-1}; t_0 = -3*m_0 + 4*m_1 - m_2; t_l = 3*m_l - 4*m_{l-1} + m_{l-2} (l = Se - 1); t = t / |t|;
 *            cos_j = t.x*e.x + t.y*e.y; any cos_j not > 0.25 (NaN included): steep.  Normal n = (-t.y, t.x).
 *  5. half thickness  var = n.x*n.x*cxx + 2*n.x*n.y*cxy + n.y*n.y*cyy, h = (sqrt(12*max(var, 0) + 1) - 1) / 2 (r full pixel rows
 *            give (r - 1) / 2, the point extent `mini_box` measures); the end slabs are under-filled: h_0 = h_1, h_l = h_{l-1}.
 *  6. knots 0 .. Se + 1: knot i, 1 <= i <= Se, is (m, t, n, h) of slab i - 1; the end knots take t, n, h of their neighbour and
 *            c_0 = m_0 - t_0*((sw / 2) / cos_0), c_last = m_l + t_l*((sw / 2) / cos_l).
 *  7. unclip  T_i = c_i - n_i*h_i, B_i = c_i + n_i*h_i; A2 = sum of x_i*y_{i+1} - x_{i+1}*y_i and Lp = sum of |q_{i+1} - q_i| around
 *            T_0 .. T_last, B_last .. B_0 (from 0, in that order); d = |A2| / 2 * ratio / Lp; c_0 -= d*t_0, c_last += d*t_last,
 *            every h_i += d; T and B again.
 *  8. fold   every cell (T_i, T_{i+1}, B_{i+1}, B_i) strictly convex: with q0..q3 its corners, all four
 *            (q_{j+1} - q_j).x*(q_{j+2} - q_{j+1}).y - (q_{j+1} - q_j).y*(q_{j+2} - q_{j+1}).x > 0 (y down); otherwise folded.  It is
 *            the condition under which the bilinear cell map of mr_strip_crop is one-to-one.
 *  9. scale  x / W * dest_w, y / H * dest_h; not rounded, not clamped.
 * 3 <= slabs <= MR_RIBBON_MAX_SLABS, 0 <= ratio <= 1e6 (1.5 is the boxes' unclip ratio), the shapes mr_db_boxes takes; MR_ERR_ARG
 * otherwise, nothing launched. */
#define MR_RIBBON_MAX_SLABS 16
#define MR_RIBBON_MAX_KNOTS 18
int mr_db_ribbons_ws_bytes(int N, int K, long long* bytes);
int mr_db_ribbons(const int* dest, int N, int H, int W, int K, int slabs, double ratio, const void* ws, void* rws,
                  double* ribbons, int* knots, int* why, hipStream_t stream);

/* ---- DB detector metrics (concern/icdar2015_eval/detection/iou.py:13-179 `evaluate_image` for quadrilaterals, the
 * evaluator of structure/measurers/quad_measurer.py).  All arithmetic float64.  gt f64 [N][G][4][2] / det f64 [N][D][4][2]
 * padded per image, gt_count / det_count i32 [N] = used slots.
 * mr_quad_iou: gt_valid i32 [N][G], det_valid i32 [N][D] (1 = area non-zero and neither pair of opposite edges intersects
 * or touches), gt_area / det_area f64 (absolute shoelace area), inter f64 [N][G][D] (area of the intersection, exact for
 * convex and concave quads of either orientation), iou f64 [N][G][D] = inter / (gt_area + det_area - inter).  Every
 * element is written; padding slots and pairs with an invalid member get 0.
 * mr_quad_match: one image per wavefront; indices are positions in the compacted lists of VALID quads, original order.
 * gt_ignore i32 [N][G]: a valid gt with ignore != 0 is don't-care; a valid det d is don't-care iff a don't-care gt g has
 * inter[g][d] / det_area[d] > area_precision_constraint; going through g ascending and d ascending, (g, d) match iff both
 * are unmatched, both care and iou[g][d] > iou_constraint (the reference's greedy order).  counts i32 [N][4] = (gtCare,
 * detCare, detMatched, valid gts); scores f64 [N][3] = (precision, recall, hmean) by the reference's case analysis;
 * match_det i32 [N][G] = det matched to gt g or -1 (-1 in unused slots); gt_dontcare i32 [N][G] / det_dontcare i32 [N][D]
 * flags (0 in unused slots).  G and D up to 1024 each, MR_ERR_UNSUPPORTED beyond. */
int mr_quad_iou(const double* gt, const int* gt_count, const double* det, const int* det_count, int N, int G, int D,
                int* gt_valid, int* det_valid, double* gt_area, double* det_area, double* inter, double* iou,
                hipStream_t stream);
int mr_quad_match(const int* gt_valid, const int* det_valid, const int* gt_ignore, const double* det_area, const double* inter,
                  const double* iou, int N, int G, int D, double iou_constraint, double area_precision_constraint, int* counts,
                  double* scores, int* match_det, int* gt_dontcare, int* det_dontcare, hipStream_t stream);
/* mr_poly_iou: the tables of mr_quad_iou for SIMPLE POLYGONS of 3 .. V vertices each (curved text: a ribbon's outline, the 14
 * points of CTW1500, Total-Text), so that mr_quad_match runs on them unchanged.  gt f64 [N][G][V][2], gt_verts i32 [N][G] = vertices of
 * each polygon (those at and beyond it are padding), gt_count i32 [N] = used slots; det / det_verts / det_count alike with D.
 * 3 <= V <= MR_POLY_MAX_VERTS: MR_ERR_ARG below, MR_ERR_UNSUPPORTED above (refused, not truncated).  All arithmetic float64, every
 * product and sum rounded on its own (tests/_poly_eval_ref.py restates it).  Every element of the six outputs is written; padding
 * slots, polygons that are not valid and pairs with such a member get 0.
 * Validity (shapely's `is_valid and is_simple` restated for a ring of m vertices, edge e = v_e -> v_(e+1 mod m)): m in 3 .. V, and
 *   1. A2 = sum over e = 0, 1, ... of x_e*y_(e+1) - x_(e+1)*y_e, added in that order from 0, has 0 < |A2| < inf (area = |A2| / 2);
 *   2. no two vertices are equal;
 *   3. no two NON-ADJACENT edges share a point (closed segments: crossing, touching or overlapping);
 *   4. no edge folds back onto the one before it: not (orient2(v_e, v_(e+1), v_(e+2)) == 0 and
 *      (v_e - v_(e+1)) . (v_(e+2) - v_(e+1)) > 0) -- the shared vertex is the only point two adjacent edges may have in common.
 *   For m = 4 this is mr_quad_iou's rule (a fold or a repeated vertex of a 4-gon puts a vertex on the opposite edge).
 * Intersection area, exact for every pair of valid polygons, convex or not, either orientation, any start vertex; a pair whose
 * bounding boxes are disjoint is exactly 0 and nothing more is computed:
 *   1. translate: P_i = p_i - p_0 (gt), Q_j = q_j - p_0 (det), BOTH by the gt's first vertex, before any product;
 *   2. fans: S_i = (P_0, P_(i+1), P_(i+2)), i = 0 .. m-3, C_j = (Q_0, Q_(j+1), Q_(j+2)), j = 0 .. n-3; o = orient2 of the triangle
 *      as listed; o == 0: the triangle is skipped; o < 0: its last two vertices are swapped (stored counter-clockwise);
 *   3. term t = i*(n-2) + j: sign(o_i)*sign(o_j) * area(S_i and C_j), the area by clipping S_i with the three edges of C_j
 *      (Sutherland-Hodgman, as for quads); 0 without clipping when the triangles' boxes are disjoint.  The signed fans add up to each
 *      polygon's indicator times its orientation, and the absolute value below removes the product of the two orientations;
 *   4. order: a_l = the terms t = l, l + 64, l + 128, ... added in that order from 0, l = 0 .. 63; then for step = 32, 16, 8, 4, 2, 1:
 *      a_l = a_l + a_(l + step) for l < step; inter = |a_0|; iou = inter / (gt_area + det_area - inter). */
#define MR_POLY_MAX_VERTS 64
int mr_poly_iou(const double* gt, const int* gt_verts, const int* gt_count, const double* det, const int* det_verts,
                const int* det_count, int N, int G, int D, int V, int* gt_valid, int* det_valid, double* gt_area,
                double* det_area, double* inter, double* iou, hipStream_t stream);

/* ---- DB detector training targets (data/processes/make_seg_detection_data.py:21-99 `MakeSegDetectionData` and
 * data/processes/make_border_map.py:24-120 `MakeBorderMap` for quadrilaterals; the batch of decoders/seg_detector_loss.py).
 * All geometry float64, pixel (x, y) = the integer point (x, y).  polys f64 [N][G][4][2] padded per image, count i32 [N] =
 * used slots, ignore_in i32 [N][G] = the labels' ignore tags.
 * Per used slot: clip to [0, W-1] x [0, H-1]; a = `polygon_area`; points reordered (0, 3, 2, 1) if a > 0; ignored if
 * ignore_in, |a| < 1, min(height, width) < min_text_size, or no pixel is inside the polygon (even-odd) at squared distance
 * >= D^2 from its boundary, D = |a| (1 - shrink_ratio^2) / perimeter (the restatement of `shrinked == []`).
 * records: scratch of N * G * mr_sizeof_db_record() bytes (the prep kernel's per-slot result; may be NULL when G == 0).
 * ignore_out i32 [N][G]: the final flags (0 in unused slots); dist f64 [N][G]: D of a kept polygon, else 0.
 * gt f32 [N][1][H][W]: 1 inside a kept polygon at d^2 >= D^2; mask f32 [N][H][W]: 0 inside, or within half a pixel of an
 * edge of, an ignored polygon's truncated points, else 1; thresh_mask f32 [N][H][W]: 1 inside a kept polygon or at d^2 <= D^2;
 * thresh_map f32 [N][H][W] = c * (float)(thresh_max - thresh_min) + (float)thresh_min, c = max(0, max_k 1 - min(1, e_k / D_k))
 * over the kept polygons whose box [rnd(min - D), rnd(max + D)] holds the pixel, e_k = `MakeBorderMap.distance` minimised
 * over the non-degenerate edges.  Every element of the six outputs is written (no memset needed); no atomics, deterministic.
 * G up to 1024, MR_ERR_UNSUPPORTED beyond; G == 0 is valid. */
int mr_sizeof_db_record(void);
int mr_db_targets(const double* polys /* [N][G][4][2] */, const int* count /* [N] */,
                  const int* ignore_in /* [N][G] */, int N, int G, int H, int W,
                  double min_text_size, double shrink_ratio, double thresh_min, double thresh_max,
                  void* records, int* ignore_out /* [N][G] */, double* dist /* [N][G], D or 0 */,
                  float* gt, float* mask, float* thresh_map, float* thresh_mask,
                  hipStream_t stream);

/* ---- Attention-GRU decoder step kernels (decoders/attention_decoder.py:146-231; the GEMMs use mr_gemm_nt/tn) ----- */
int mr_attn_step_fwd(int dtype, const void* hproj, const void* eproj, const float* v, const void* enc, float* weights,
                     void* context, int N, int T, int Hd, int Ep, hipStream_t stream);
/* deproj / denc (f32, shared by all steps of a sequence) are accumulated (+=); dv (f32) is accumulated atomically */
int mr_attn_step_bwd(int dtype, const void* dcontext, const float* dweights, const void* hproj, const void* eproj,
                     const float* v, const void* enc, const float* weights, void* dhproj, float* deproj, float* dv,
                     float* denc, int N, int T, int Hd, int Ep, hipStream_t stream);
int mr_gru_gates_fwd(int dtype, const void* gi_a, const void* gi_b, const void* gh, const void* h, void* hnew,
                     float* save, int N, int H, hipStream_t stream);
int mr_gru_gates_bwd(int dtype, const void* dhnew, const float* save, const void* gh, const void* h, void* dgi,
                     void* dgh, void* dh, int N, int H, hipStream_t stream);
int mr_nll_step_fwd(int dtype, const void* logits, int ldl, const long long* target, long long tstride,
                    const float* mask, float* lp, float* loss, long long* argmax, int N, int C, int accumulate,
                    int softmax_out, hipStream_t stream);
/* training decode loop: mr_nll_step_fwd (log-probs) that also writes the word index fed to the NEXT step,
 * feed_idx[n] = *feed_flag ? target[n] : arg-max[n].  feed_flag points to ONE int in device memory: the teacher-forcing coin of
 * this step (decoders/attention_decoder.py:107-110) -- a device value, so a replayed hipGraph follows the coins of the current
 * step, not those of the step that was captured; null = arg-max feedback. */
int mr_nll_step_feed_fwd(int dtype, const void* logits, int ldl, const long long* target, long long tstride,
                         const float* mask, float* lp, float* loss, long long* argmax, const int* feed_flag,
                         long long* feed_idx, int N, int C, int accumulate, hipStream_t stream);
int mr_nll_step_bwd(int dtype, const float* gloss, const float* lp, const long long* target, long long tstride,
                    const float* mask, void* dlogits, int ldd, int N, int C, hipStream_t stream);
/* word embedding of the attention decoder (decoders/attention_decoder.py:187-193): out[n, :D] = table[idx[n]] cast to
 * `dtype`, columns D..ldo-1 zeroed; backward scatter-adds into the f32 table gradient */
int mr_embed_rows_fwd(int dtype, const long long* idx, const float* table, void* out, int N, int V, int D, int ldo,
                      hipStream_t stream);
int mr_embed_rows_bwd(int dtype, const long long* idx, const void* dout, float* dtable, int N, int V, int D, int ldo,
                      hipStream_t stream);
/* round-3 decode loop (one autograd Function for the 32 steps, megreader_amd/decoders/attention_decoder.py): the same math as
 * the step kernels above with strided operands -- hproj / gh are column slices (leading dimensions ldh / ldgh) of ONE stacked
 * GEMM output per step, gi_a rows are gathered from a [classes, 3H] table through idx (nullable), the three consumers of h'
 * are summed inside mr_gru_bwd2 (dh_a / dh_b / dh_c nullable), mr_attn_bwd2 runs on a (N, Hd/64) grid and leaves the
 * encoder-side gradient to ONE mr_attn_denc launch after the loop (denc[n,t,c] = sum_s weights[s,n,t] * dcontext[s,n,c]),
 * mr_rows_scatter_add is the gradient of the table gather (f32 atomics into dtable [V][D]). */
int mr_attn_fwd2(int dtype, const void* hproj, long long ldh, const void* eproj, const float* v, const void* enc,
                 float* weights, void* context, int N, int Tn, int Hd, int Ep, hipStream_t stream);
int mr_attn_bwd2(int dtype, const void* dcontext, const float* dweights, long long ldw, const void* hproj, long long ldh,
                 const void* eproj, const float* v, const void* enc, const float* weights, void* dhproj, long long lddh,
                 float* deproj, float* dv, int N, int Tn, int Hd, int Ep, hipStream_t stream);
int mr_attn_denc(int dtype, const float* weights, const void* dcontext, void* denc, int S, int N, int Tn, int Ep,
                 hipStream_t stream);
int mr_gru_fwd2(int dtype, const void* gi_a, long long lda, const long long* idx, const void* gi_b, const void* gh,
                long long ldgh, const void* h, void* hnew, float* save, int N, int H, hipStream_t stream);
int mr_gru_bwd2(int dtype, const void* dh_a, const void* dh_b, const void* dh_c, const float* save, const void* gh,
                long long ldgh, const void* h, void* dgi, void* dgh, long long lddgh, void* dh_prev, int N, int H,
                hipStream_t stream);
int mr_rows_scatter_add(int dtype, const long long* idx, const void* rows, long long ldr, float* dtable, int R, int V,
                        int D, hipStream_t stream);

/* Persistent forward of the attention-GRU decode loop (reference decoders/attention_decoder.py:84-118 around
 * AttentionRNNCell :146-231): all S steps in ONE launch of ceil(N/16) x 32 co-resident workgroups; the stacked hidden projection
 * [4H][H] (attention hidden half + W_hh), the context columns of W_ih and the encoder rows stay in registers / LDS for the whole
 * sequence and the three per-step hand-offs (partial energies -> owners, contexts, h') go through tagged 8-byte granules
 * (decode_persist.hip).  bf16 only, H = 512.  cat_w [4H][H], cat_b [4H] f32 (nullable), ic_w [3H][ldic], G = word table
 * [classes][ldG >= 3H] gathered by idx [S][N] (the word fed to each step), eproj [N][T][H], enc [N][T][Ep], v [H] f32.
 * Writes what the per-step path (mr_gemm_nt + mr_attn_fwd2 + mr_gemm_gru_fwd) saves for the backward: H_all [S+1][N][H]
 * (H_all[0] = the initial state, read), HC_all [S][N][4H], W_att [S][N][T] f32, CTX_all [S][N][Ep], SAVE_all [S][N][3H] f32.
 * flags null: every step is fed the word idx[s] (teacher forcing).  flags [S] int32 on the device (the per-step coins of
 * attention_decoder.py:107-110): where flags[s] == 0, step s + 1 is fed the arg-max of step s's output layer out_w [C][H] / out_b
 * (f32, nullable), C <= 256, first index on ties as mr_out_nll_fwd -- and the kernel WRITES that word to idx[s + 1].
 * ws: exchange workspace of mr_decode_persist_ws_bytes(N) bytes, zeroed by the call (ws_bytes > 0) or by the caller (pass the
 * size NEGATIVE).  A hand-off that times out records a code in the status word behind the workspace and poisons h' with NaN. */
int mr_decode_persist_ok(int dtype, int N, int T, int H, int Ep);   /* host only; 0 also when mr_tuning.decode_persist = 0 or the
                                                                        current device has fewer CUs than the launch has workgroups */
long long mr_decode_persist_ws_bytes(int N);                        /* host only */
int mr_decode_persist_fwd(const void* cat_w, const float* cat_b, const void* ic_w, long long ldic, const void* G, long long ldG,
                          long long* idx, const int* flags, const void* out_w, const float* out_b, int C, const void* eproj,
                          const void* enc, const float* v, void* H_all, void* HC_all, float* W_att, void* CTX_all,
                          float* SAVE_all, void* ws, long long ws_bytes, int S, int N, int T, int Ep, hipStream_t stream);
/* ... and its backward: all S steps in reverse in one launch -- what mr_gemm_gru_bwd / mr_gru_bwd2 + mr_gemm_nt + mr_attn_bwd2 compute
 * per step (N <= 32).  cat_wt [H][4H] and ic_wt [Ep][ldict >= 3H] are the TRANSPOSED weight images (row = output of the backward
 * GEMM, K = stacked column / gate unit); DHO_all [S][N][H] = gradient of every h' from the output layer; ga (nullable) = gradient
 * of the attention weights, element (n, s, t) at ga[n * ldga + s * T + t].  Writes DGI_all [S][N][3H], DHC_all [S][N][4H],
 * DCTX_all [S][N][Ep], deproj [N][T][H] (f32, plain stores: the per-step path accumulates into it), ADDS into dv [H] (f32) and,
 * when denc is not null, writes denc [N][T][Ep] = sum_s W_att[s] dctx[s] (what mr_attn_denc computes after the per-step loop). */
int mr_decode_persist_bwd_ok(int dtype, int N, int T, int H, int Ep);   /* host only */
long long mr_decode_persist_bwd_ws_bytes(int N);                        /* host only */
int mr_decode_persist_bwd(const void* cat_wt, const void* ic_wt, long long ldict, const void* eproj, const void* enc,
                          const float* v, const void* H_all, const void* HC_all, const float* W_att, const float* SAVE_all,
                          const void* DHO_all, const float* ga, long long ldga, void* DGI_all, void* DHC_all, void* DCTX_all,
                          float* deproj, float* dv, void* denc, void* ws, long long ws_bytes, int S, int N, int T, int Ep,
                          hipStream_t stream);
/* ... and the GREEDY form of the forward for inference (the eval loop of attention_decoder.py:84-118): the same kernel, compiled
 * without the stores of the backward's buffers.  Step 0 is fed `start_word` for every row, step s + 1 the arg-max of step s's
 * output layer out_w [C][H] / out_b (f32, nullable), 1 <= C <= 256, first index on ties; no idx, no flags.  h0 [N][H] is the
 * initial state.  Writes pred[n * ldp + s] (int32, ldp >= S) for EVERY step s < S -- the last step's arg-max is one more
 * best-class sweep behind the loop -- and, only when H_all is not null, H_all [S+1][N][H] ([0] = h0).  Rows of a batch group
 * whose hand-off timed out get -1 in pred from that step on (status word as above).  ws / ws_bytes as mr_decode_persist_fwd
 * (mr_decode_persist_ws_bytes(N)).  A bad shape is refused before any launch. */
int mr_decode_greedy_ok(int dtype, int N, int T, int H, int Ep, int C);   /* host only: mr_decode_persist_ok and 1 <= C <= 256 */
int mr_decode_greedy_fwd(const void* cat_w, const float* cat_b, const void* ic_w, long long ldic, const void* G, long long ldG,
                         const void* out_w, const float* out_b, int C, const void* eproj, const void* enc, const float* v,
                         const void* h0, int start_word, int* pred, long long ldp, void* H_all, void* ws, long long ws_bytes,
                         int S, int N, int T, int Ep, hipStream_t stream);
/* The reference's early stop, applied afterwards: pred int32 [N][ldp], S columns used.  With t* = the first column in which all N
 * rows equal `blank`, every element of the columns > t* becomes `blank`; no such column: nothing changes.  (No step before t*
 * depends on the break, so decoding all S steps and trimming gives the loop's tensor.)  One workgroup; any N. */
int mr_decode_greedy_trim(int* pred, long long ldp, int N, int S, int blank, hipStream_t stream);

/* ---- Round-4 decode-step fusions (csrc/gemm_skinny.hip): the element-wise GRU kernels in the epilogue of the M <= 32 GEMM next
 *      to them, the output layer + log-softmax + NLL + arg-max feedback as one kernel.  Same reference lines as above
 *      (attention_decoder.py:92-115,195-231); forward chain per step 6 -> 4 launches, backward 4 -> 3. ---------------------- */
/* mr_gemm_nt(ctx, w_ic) + mr_gru_fwd2 in one launch: gi_c = ctx [M, K] * w_ic [3H, K]^T stays in f32 and feeds the GRU cell of
 * the workgroup's 16 hidden units.  G: word table rows gathered by idx (null: row m), leading dimension ldG >= 3H; gh: the
 * hidden projection with its bias, leading dimension ldgh; h / hnew [M, H]; save f32 [M, 3H] (r, z, n).  M <= 32. */
int mr_gemm_gru_fwd(int dtype, const void* ctx, long long ldc, const void* w_ic, long long ldw, const void* G, long long ldG,
                    const long long* idx, const void* gh, long long ldgh, const void* h, void* hnew, float* save, int M, int H,
                    int K, hipStream_t stream);
/* mr_gemm_nt(dhc, w_t) + mr_gru_bwd2 in one launch: dh_a = dhc [M, K] * w_t [H, K]^T is never stored; dh_b / dh_c nullable;
 * dh_prev may alias dh_b.  Outputs as mr_gru_bwd2. */
int mr_gemm_gru_bwd(int dtype, const void* dhc, long long lda, const void* w_t, long long ldw, const void* dh_b,
                    const void* dh_c, const float* save, const void* gh, long long ldgh, const void* h, void* dgi, void* dgh,
                    long long lddgh, void* dh_prev, int M, int H, int K, hipStream_t stream);
/* mr_gemm_nt(h, W, bias) + mr_nll_step_feed_fwd in one launch (one workgroup per sample; the logits stay in f32 and are not
 * stored): lp f32 [N, C] = log_softmax, loss[n] (+)= -lp[n, target] * mask[n], argmax, feed_idx[n] = *feed_flag ? target[n] :
 * argmax[n] (feed_flag / feed_idx / loss / argmax / mask / bias nullable).  C <= 256. */
int mr_out_nll_fwd(int dtype, const void* h, long long ldh, const void* W, long long ldw, const float* bias,
                   const long long* target, long long tstride, const float* mask, float* lp, float* loss, long long* argmax,
                   const int* feed_flag, long long* feed_idx, int N, int C, int K, int accumulate, hipStream_t stream);

/* eval head: softmax over classes of logits [T,N,C] -> f32 [N,C,1,T] (decoders/crnn.py:101-104) */
int mr_softmax_nc1t(int dtype, const void* logits, int ldl, float* out, int T, int N, int C, hipStream_t stream);

/* ---- evaluation decode + metrics on the GPU ------------------------------------------------
 * mr_ctc_greedy_decode: structure/representers/ctc_representer.py:20-34.  pred[n,c,t] at pred + n*sn + c*sc + t*st
 *   (element strides; dtype 0 = f32, 1 = bf16, 2 = f64).  argmax over c (first index on ties); a symbol is skipped if
 *   it equals `previous` or is `unknown` (an unknown does not update `previous`); emitted if != blank.
 *   out: i32 [N, T] blank padded; out_len (nullable): i32 [N] number of emitted symbols.
 * mr_ctc2d_greedy_decode: structure/representers/ctc_representer2d.py:27-51.  classify[n,c,h,w], mask[n,0,h,w] f32
 *   with element strides; per column h* = argmax_h max_c(classify*mask), c* = argmax_c at h*; same collapse.
 * mr_seq_measure: structure/measurers/sequence_recognition_measurer.py:66-72,101-112 on id sequences (blank / unknown
 *   dropped as concern/charsets.py:60-62 does; fold: nullable id -> canonical id table for `.upper()`):
 *   acc[n] = sequences equal; ed[n] = Levenshtein distance; label_len[n] = symbols of the label;
 *   score[n] (f64) = 0 if len(label) == 0 else 1 - min(len, ed) / len.  Every output is exact for any number of
 *   symbols per row: rows with both sequences <= 63 symbols take one anti-diagonal pass in registers, longer rows a
 *   row-by-row pass in LDS (same launch).  The LDS holds both sequences whole, so S and S2 above MR_SEQ_MEASURE_MAX
 *   are refused with MR_ERR_ARG and nothing is written. */
#define MR_SEQ_MEASURE_MAX 4096
int mr_ctc_greedy_decode(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T,
                         int blank, int unknown, int* out, int* out_len, hipStream_t stream);
int mr_ctc2d_greedy_decode(const float* classify, long long cn, long long cc, long long ch, long long cw,
                           const float* mask, long long mn, long long mh, long long mw, int N, int C, int H, int W,
                           int blank, int unknown, int* out, int* out_len, hipStream_t stream);
int mr_seq_measure(const int* labels, int S, const int* preds, int S2, int N, int blank, int unknown, const int* fold,
                   int* acc, int* ed, int* label_len, double* score, hipStream_t stream);

/* ---- input pipeline on the GPU ----------------------------------------------------------------
 * mr_resize_normalize: data/processes/resize_image.py:29-38,48-53 (cv2.resize of the float32 image, INTER_LINEAR;
 *   modes "resize" and "pad") fused with data/processes/normalize_image.py:8-17 (-= RGB_MEAN in double, /= 255 in f32,
 *   HWC -> CHW).  src: packed uint8 HWC (3 channel) images; desc: device array of mr_img_desc (mr_sizeof_img_desc()
 *   bytes each); dst: f32 [N,3,H,W].  The kernel is in csrc/image_sample.hip with mr_warp_normalize and mr_quad_crop, which
 *   share its normalising store.
 * mr_encode_labels: concern/charsets.py:37-58 + data/processes/make_recognition_label.py:11-24.  codepoints: i32
 *   UTF-32 text of all strings back to back, offsets: i64 [N+1]; table_cp (sorted) / table_id: the charset's
 *   codepoint -> id map (case folding baked in by the host); label: i32 [N, max_size] zero padded,
 *   length: i32 [N] = min(len, max_size). */
typedef struct mr_img_desc {
  long long offset;             /* byte offset of the image's first pixel in the packed source buffer */
  int h, w, pitch, dst_w;       /* rows, columns, bytes per row; columns of the resized image inside the canvas (== W for "resize") */
  double scale_x, scale_y;      /* cv2: scale = 1. / ((double)dsize / ssize), evaluated by the host (not ssize / dsize, which rounds differently) */
} mr_img_desc;
int mr_sizeof_img_desc(void);
int mr_resize_normalize(const unsigned char* src, const void* desc, int N, int H, int W, double mean0, double mean1,
                        double mean2, float* dst, hipStream_t stream);
int mr_encode_labels(const int* codepoints, const long long* offsets, int N, int max_size, const int* table_cp,
                     const int* table_id, int ntab, int unknown, int* label, int* length, hipStream_t stream);

/* ---- Baseline JPEG decode (csrc/jpeg.hip, csrc/jpeg_plan.h): the "decode" in front of the input pipeline.  A batch of encoded
 * files goes to the device as bytes; the host only reads their marker segments (mr_jpeg_plan: one call per batch, no allocation,
 * no GPU call) and the device does the entropy decode, dequantisation, inverse DCT, chroma upsampling and colour conversion.
 * The pixels are bit-identical to the default decode of libjpeg / libjpeg-turbo (slow-integer IDCT, triangle upsampling,
 * 16-bit fixed-point YCbCr -> RGB), which is what PIL and cv2.imdecode return.
 * Supported on the device: SOF0 (baseline, 8-bit, Huffman), 1 or 3 components in one interleaved scan, luma sampling 1x1, 2x1
 * or 2x2 with chroma 1x1, 8-bit quantisation tables, YCbCr (JFIF, Adobe transform 1, or unmarked) or grayscale.  Everything else
 * -- progressive, arithmetic, 12-bit, 4 components, Adobe transform 0, multi-scan, other sampling, bytes that do not start with
 * SOI -- is MR_JPEG_UNSUPPORTED (decode it on the host); a file that starts as a JPEG and breaks the syntax is MR_JPEG_CORRUPT.
 *
 * mr_jpeg_plan fills images[n] and the work items: an image without a restart interval is one item, an image with one is one item
 * per interval (the host finds the RSTn markers with a byte scan).  One wavefront decodes one item, so restart markers are the
 * only parallelism inside one image.  totals[4] = {items needed, bytes of the blob buffer, of the workspace, of the output}: the
 * caller copies blob i to blob_off of ONE buffer (offsets are 16-byte aligned, all blobs are laid out whatever their status) and
 * allocates the other two.  When totals[0] > max_items the item list is incomplete: call again with room for totals[0].
 * On MR_JPEG_OK every offset of the plan lies inside its buffer. */
#define MR_JPEG_OK 0
#define MR_JPEG_UNSUPPORTED 1
#define MR_JPEG_CORRUPT 2
typedef struct mr_jpeg_image {
  int status, h, w, ncomp;
  int hs, vs;                     /* luma sampling factors (chroma is 1x1; a grayscale image reports 1x1) */
  int mcu_w, mcu_h;               /* MCUs per row, MCU rows */
  int restart;                    /* restart interval in MCUs, 0: none */
  int first_item, n_items;        /* this image's work items */
  int reserved0;
  long long blob_off, blob_len;   /* the blob inside the blob buffer */
  long long scan_off, scan_len;   /* the entropy-coded segment inside the blob */
  long long plane_off[3];         /* uint8 component planes inside the workspace, padded to whole MCUs */
  int plane_pitch[3], plane_rows[3];
  long long out_off;              /* first output byte: uint8 [h][w][3], pitch exactly w * 3 */
  int comp_tq[3], comp_td[3], comp_ta[3];   /* per component: quantisation table 0..3, DC table 0..1, AC table 0..1 */
  int reserved1;
  int quant[64];                  /* 4 tables x 64 BYTES in memory order, coefficients in zigzag order */
  int huff_maxcode[64];           /* [DC0, DC1, AC0, AC1][code length - 1]: the largest code of that length, -1: none */
  int huff_valoff[64];            /* same index: (index of the first symbol of that length) - (its code) */
  int huff_sym[256];              /* 4 tables x 256 BYTES in memory order: the symbols by increasing code */
} mr_jpeg_image;
typedef struct mr_jpeg_item {
  int image, mcu0, nmcu, reserved;   /* MCUs mcu0 .. mcu0 + nmcu - 1 of that image, DC predictors starting at 0 */
  long long off, len;                /* their stuffed bytes inside the blob; no marker inside */
} mr_jpeg_item;
int mr_sizeof_jpeg_image(void);
int mr_sizeof_jpeg_item(void);
int mr_jpeg_plan(int n, const void* const* blobs, const long long* lens, mr_jpeg_image* images, mr_jpeg_item* items,
                 long long max_items, long long* totals);
/* blobs_dev: the blob buffer; plan_dev: the n_images mr_jpeg_image followed by the n_items mr_jpeg_item, as mr_jpeg_plan wrote
 * them (16-byte aligned); workspace, out: totals[2] and totals[3] bytes; status: i32 [n_images], written by the call (the plan's
 * status, raised to MR_JPEG_CORRUPT when an item meets an invalid code or runs out of bytes before its last MCU -- such an image's
 * pixels are unspecified, every other image is unaffected).  rgb: 0 writes B, G, R per pixel (cv2's order), 1 writes R, G, B.
 * Only bytes [out_off, out_off + h*w*3) of OK images are written.  Three launches on `stream`, no host synchronisation. */
int mr_jpeg_decode(const void* blobs_dev, const void* plan_dev, int n_images, int n_items, void* workspace, void* out,
                   int* status, int rgb, hipStream_t stream);

/* ---- Parallel decode inside one long work item (csrc/jpeg_split.hip): a photo without restart markers is ONE item, which one
 * wavefront decodes serially.  mr_jpeg_plan_split, host only and after mr_jpeg_plan, describes every item longer than split_above
 * bytes in splits[] (items[i].reserved becomes 1 + its index there; the single-wave kernel skips such items) and grows totals[2],
 * the workspace, by their regions.  The item is cut into n_sub sub-sequences of subseq_bytes UNSTUFFED bytes (a multiple of 4 in
 * [16, 1024]; n_sub = ceil(len / subseq_bytes) from the stuffed length, an upper bound -- sub-sequences behind the data are
 * empty), 256 per workgroup.  *n_splits is the number of such items; when it exceeds max_splits nothing was written: call again
 * with room.  With no item above split_above the plan is left byte for byte as it was.
 * mr_jpeg_decode_split = mr_jpeg_decode + the split stages between the status kernel and the colour kernel: unstuff, decoder
 * synchronisation (1 + (largest n_wg - 1) launches: a sub-sequence is re-decoded until the state it was decoded from equals the
 * state its predecessor produced, so every entry state is the serial decoder's), block-offset scan, coefficient write, DC prefix
 * sum, inverse DCT.  splits_host / splits_dev: the same n_splits entries on the host (launch sizes) and on the device, 16-byte
 * aligned.  Pixels and status equal mr_jpeg_decode's on the same stream of bytes.  n_splits == 0: exactly mr_jpeg_decode's three
 * launches.  No host synchronisation, no waiting between workgroups. */
typedef struct mr_jpeg_split {
  int item, image;
  int subseq_bytes, n_sub, n_wg;     /* n_wg = ceil(n_sub / 256) */
  int n_blocks;                      /* blocks the item holds: nmcu * blocks_per_mcu */
  int blocks_per_mcu, reserved;
  long long meta_off;                /* workspace offsets, 16-byte aligned.  meta: int [4] = unstuffed bytes, blocks completed */
  long long raw_off, raw_bytes;      /* the unstuffed bytes, zero from the last one up to raw_bytes */
  long long in_off, exit_off;        /* per sub-sequence {u32 bit position; u32 blocks << 16 | block slot << 8 | zigzag index} */
  long long wg_exit_off;             /* [2][n_wg] such states */
  long long block_off;               /* int [n_sub]: exclusive prefix sum of completed blocks */
  long long coef_off, coef_bytes;    /* int dc[n_blocks] (padded to 16 bytes), short coef[n_blocks][64], zigzag order */
} mr_jpeg_split;
int mr_sizeof_jpeg_split(void);
int mr_jpeg_plan_split(int n_images, const mr_jpeg_image* images, mr_jpeg_item* items, long long n_items, long long split_above,
                       int subseq_bytes, mr_jpeg_split* splits, long long max_splits, long long* totals, long long* n_splits);
int mr_jpeg_decode_split(const void* blobs_dev, const void* plan_dev, int n_images, int n_items, const mr_jpeg_split* splits_host,
                         const void* splits_dev, int n_splits, void* workspace, void* out, int* status, int rgb,
                         hipStream_t stream);

/* ---- DB detector augmentation (csrc/image_sample.hip): the image half of data/processes/augment_data.py
 * (`AugmentDetectionData`: Fliplr, Affine rotate, Resize), data/processes/random_crop_data.py (`RandomCropData`) and
 * data/processes/normalize_image.py in ONE bilinear pass.  The host composes the chain into one affine map per image
 * (megreader_amd/data/detection_augment.py); the kernel samples the decoded uint8 HWC source once along it and writes the
 * normalised f32 [N][3][H][W] canvas.  Canvas pixel (u, v), v < dst_h and u < dst_w:
 *   uc = min(max(u, cu0), cu1), vc = min(max(v, cv0), cv1)
 *   x = a[0]*uc + a[1]*vc + a[2], y = a[3]*uc + a[4]*vc + a[5]     (float64, left to right, every product and sum rounded)
 *   ix = floor(x), fx = (float)(x - ix); iy = floor(y), fy = (float)(y - iy)
 *   p00 = src(ix, iy), p01 = src(ix + 1, iy), p10 = src(ix, iy + 1), p11 = src(ix + 1, iy + 1) as float; a tap outside
 *   [0, src_w) x [0, src_h), or outside the uploaded window, is 0
 *   top = p00*(1 - fx) + p01*fx, bot = p10*(1 - fx) + p11*fx, val = top*(1 - fy) + bot*fy        (float32, no fma)
 *   dst[n][c][v][u] = (float)((double)val - mean[c]) / 255.f                         (as mr_resize_normalize ends)
 * Every other canvas pixel gets the normalised value of a zero pixel; every element of dst is written.  With a = identity,
 * the clamp and the valid region the whole canvas, the result equals mr_resize_normalize at identity scale bit for bit.
 * The kernel reads only bytes src[offset + r*pitch + 3*k + c], 0 <= r < win_h, 0 <= k < win_w: the host may upload the
 * window alone. */
typedef struct mr_warp_desc {
  long long offset;             /* byte offset of the uploaded window's first pixel in the packed source buffer */
  int pitch;                    /* bytes per row of the uploaded window (>= 3 * win_w) */
  int src_h, src_w;             /* the full source image: taps outside it read as pixel value 0 (imgaug cval = 0) */
  int win_x, win_y;             /* source coordinates of the window's first pixel */
  int win_h, win_w;             /* rows and columns that were uploaded; a tap outside them reads as 0 as well */
  int dst_h, dst_w;             /* valid canvas region; the rest is the zero canvas of RandomCropData */
  int reserved;                 /* 0 (keeps the doubles 8-byte aligned) */
  double cu0, cu1, cv0, cv1;    /* (u, v) is clamped to [cu0, cu1] x [cv0, cv1] before the map: the crop's replicated border */
  double a[6];                  /* canvas -> source: x = a[0]*uc + a[1]*vc + a[2], y = a[3]*uc + a[4]*vc + a[5] */
} mr_warp_desc;
int mr_sizeof_warp_desc(void);
int mr_warp_normalize(const unsigned char* src, const void* desc /* [N] */, int N, int H, int W,
                      double mean0, double mean1, double mean2, float* dst /* [N][3][H][W] */, hipStream_t stream);

/* ---- Quad crops (csrc/image_sample.hip): data/crop_file_dataset.py `ImageCropper.crop` -- getPerspectiveTransform +
 * warpPerspective of a detected quadrilateral, `ensure_horizontal`, `ResizeImage` (modes "resize" and "pad"), - RGB_MEAN,
 * / 255 -- in ONE bilinear pass from the resident uint8 HWC photos to the recogniser's f32 [M][3][H][W] batch.  The host
 * plans each crop in float64 from shapes and points only (megreader_amd/data/quad_crop.py); many crops read from a few
 * photos, so the photos are a table of their own and a crop names its photo by index.  Canvas pixel (u, v) of crop m,
 * u < dst_w (float64, left to right, every product and sum rounded on its own):
 *   cx = min(max((u + 0.5)*sx - 0.5, 0), cu1), cy = min(max((v + 0.5)*sy - 0.5, 0), cv1)      (cv2.resize's sampling point)
 *   X = h[0]*cx + h[1]*cy + h[2], Y = h[3]*cx + h[4]*cy + h[5], D = h[6]*cx + h[7]*cy + h[8];  x = X / D, y = Y / D
 *   D <= 0 (or NaN), or x or y not finite: the pixel value is 0.  Otherwise floor, (float) fractions, the four taps and the
 *   float32 blend top, bot, val of mr_warp_normalize; a tap outside [0, w) x [0, h) of its photo reads as 0
 *   (warpPerspective's BORDER_CONSTANT)
 *   dst[m][c][v][u] = (float)((double)val - mean[c]) / 255.f
 * Columns u >= dst_w, and crops whose `image` is not in [0, I), get the normalised zero pixel; every element of dst is
 * written.  The kernel reads only bytes src[offset + r*pitch + 3*k + c], 0 <= r < h, 0 <= k < w, of the photos in the table;
 * `offset` is relative to src and may be negative (a photo resident in another allocation).  The tables live in memory the
 * device reads; when `crops` is pinned host memory the entry point checks every `image` index before the launch
 * (MR_ERR_ARG), otherwise only the planner (QuadCropper.pack) and the kernel do.  M == 0 returns MR_OK without a launch. */
typedef struct mr_crop_image {
  long long offset;             /* byte offset of the photo's first pixel from src */
  int pitch;                    /* bytes per row (>= 3 * w) */
  int h, w;                     /* rows and columns */
  int reserved;                 /* 0 (pads the entry to 24 bytes) */
} mr_crop_image;
typedef struct mr_crop_desc {
  int image;                    /* index into the mr_crop_image table */
  int dst_w;                    /* valid canvas columns (mode "pad"); the rest is the zero canvas */
  double sx, sy;                /* cv2.resize scales: 1. / ((double)dst / src) of the (rotated) crop */
  double cu1, cv1;              /* the crop-frame coordinate is clamped to [0, cu1] x [0, cv1] (cv2.resize's replicated border) */
  double h[9];                  /* (rotated) crop frame -> source photo, row major, projective */
} mr_crop_desc;
int mr_sizeof_crop_image(void);
int mr_sizeof_crop_desc(void);
int mr_quad_crop(const unsigned char* src, const void* images /* [I] */, int I, const void* crops /* [M] */, int M,
                 int H, int W, double mean0, double mean1, double mean2, float* dst /* [M][3][H][W] */, hipStream_t stream);

/* ---- Strip crops (csrc/image_sample.hip): mr_quad_crop with a piecewise-bilinear mesh in the place of the homography, for words
 * that follow a curve.  A strip is `knots` rulings (top[i], bot[i]) in photo coordinates at the arc lengths s[i] of the crop frame
 * (s ascending, s[0] = 0); the host plans it from points only (megreader_amd/data/strip_crop.py).  The same photo table, output,
 * taps, blend and normalisation as mr_quad_crop.  Canvas pixel (u, v) of crop m, u < dst_w (float64, in this order, every product
 * and sum rounded on its own):
 *   cx = min(max((u + 0.5)*sx - 0.5, 0), cu1), cy = min(max((v + 0.5)*sy - 0.5, 0), cv1)         (as mr_quad_crop)
 *   i = the last knot with s[i] <= cx, at most knots - 2 (0 when there is none);  a = (cx - s[i]) / (s[i+1] - s[i]);  b = cy / hgt
 *   top = top[i]*(1 - a) + top[i+1]*a, bot = bot[i]*(1 - a) + bot[i+1]*a   (per coordinate);   (x, y) = top*(1 - b) + bot*b
 *   x or y not finite: the pixel value is 0.  Otherwise the taps and the float32 blend of mr_quad_crop.
 * Columns u >= dst_w, and crops whose `image` is not in [0, I) or whose `knots` is not in [2, 18], get the normalised zero pixel;
 * every element of dst is written.  `top` and `bot` depend on the column alone: a workgroup computes them once per column.  When
 * `strips` is pinned host memory the entry point checks `image` and `knots` of every strip before the launch (MR_ERR_ARG).
 * M == 0 returns MR_OK without a launch. */
typedef struct mr_strip_desc {
  int image;                    /* index into the mr_crop_image table */
  int dst_w;                    /* valid canvas columns (mode "pad"); the rest is the zero canvas */
  int knots;                    /* 2 .. 18 rulings */
  int reserved;                 /* 0 (keeps the doubles 8-byte aligned) */
  double sx, sy;                /* cv2.resize scales of the strip's frame, as mr_crop_desc */
  double cu1, cv1;              /* the frame coordinate is clamped to [0, cu1] x [0, cv1] */
  double hgt;                   /* the frame's height: b = cy / hgt runs from the top polyline to the bottom one */
  double s[18];                 /* arc length of the centre line at every knot */
  double top[18][2], bot[18][2];   /* the rulings' end points (x, y) in the photo */
} mr_strip_desc;
int mr_sizeof_strip_desc(void);
int mr_strip_crop(const unsigned char* src, const void* images /* [I] mr_crop_image */, int I, const void* strips /* [M] */,
                  int M, int H, int W, double mean0, double mean1, double mean2, float* dst /* [M][3][H][W] */,
                  hipStream_t stream);

/* ---- Tiled multi-scale detection (csrc/det_tiles.hip): a photo too large for one detector input is resized to a CANVAS at its
 * own scale (several canvases: several "levels"), the canvas is covered by overlapping detector-sized tiles, and the tiles'
 * probability maps are fused into one map per photo BEFORE the boxes are read, so that a word cut by a tile border comes back
 * as one box.  The host plans canvases and tiles from shapes only (megreader_amd/data/detection_tiles.py).
 *
 * The 1-D cover, applied to each axis on its own: a canvas side L, tiles of side t with halo h (t > 2h), stride s = t - 2h.
 *   L <= t: K = 1, the tile starts at 0.  Otherwise K = ceil((L - t) / s) + 1 tiles start at o_k = k*s (the last may overhang L).
 *   owner(p) of canvas coordinate p, 0 <= p < L:  0 if p < t - h, else min(K - 1, (p - h) / s)      (integer division)
 *   Every p has exactly one owner, and p - o_owner lies in [0, t): in the owner's "core", at least h from the tile's inner borders.
 *   Tile (ky, kx) of a level is entry first + ky*Kx + kx of the tile arrays.
 *
 * mr_tile_sample: ONE launch draws all T tiles of all photos and levels from the resident uint8 HWC photos (the photo table of
 * mr_quad_crop: `offset` relative to src, may be negative).  Pixel (u, v) of tile t, 0 <= u < tw, 0 <= v < th, is canvas pixel
 * (X, Y) = (x0 + u, y0 + v).  For 0 <= X < wc and 0 <= Y < hc its value is the value of mr_resize_normalize at (X, Y) of a
 * resize of photo `image` (h rows, w columns) to hc rows and wc columns, bit for bit:
 *   h == hc and w == wc:  val[c] = (float)src(X, Y)[c]                                    (cv2.resize returns a copy)
 *   otherwise  fx = (float)((X + 0.5)*scale_x - 0.5)   (the product and the sum in float64, each rounded, then one rounding to f32)
 *              sx = (int)floorf(fx), fx = fx - sx;  sx < 0: sx = 0, fx = 0;  sx >= w - 1: sx = w - 1, fx = 0;  sx1 = min(sx + 1, w - 1)
 *              fy, sy, sy1 likewise from Y, scale_y and h
 *              top = src(sx, sy)*(1 - fx) + src(sx1, sy)*fx, bot = src(sx, sy1)*(1 - fx) + src(sx1, sy1)*fx
 *              val = top*(1 - fy) + bot*fy                                                (float32, no fma)
 *   dst[t][c][v][u] = (float)((double)val[c] - mean[c]) / 255.f
 * with scale_x = 1. / ((double)wc / w) and scale_y = 1. / ((double)hc / h) evaluated by the host.  Every other pixel -- outside
 * the canvas, or of a tile whose `image` is not in [0, I) or whose wc or hc is < 1 -- is 0.0f: NOT the normalised zero pixel of
 * mode "pad", but what a detector's own zero padding supplies beyond a whole canvas, which is what makes a tiled detector
 * equal the untiled one.  Every element of dst f32 [T][3][th][tw] is written; only bytes src[offset + r*pitch + 3*k + c],
 * 0 <= r < h, 0 <= k < w, of photos in the table are read.  MR_ERR_ARG, nothing written: a null pointer with T > 0, T or I < 0,
 * th or tw < 1, T*th*tw*3 >= 2^31.  T == 0 returns MR_OK without a launch.
 *
 * mr_tile_stitch: a gather; every pixel of every fused map is written exactly once by the one thread that owns it (no atomics:
 * the bits are the same on every run).  maps: [T][th][tw], dtype MR_F32 or MR_BF16 (read as (float)).  levels: one
 * mr_stitch_level per (photo, level); photos: one mr_stitch_photo per photo, whose `levels` entries start at `first_level` and
 * are fused in that order; `base` (0 <= base < levels) names the level whose canvas is the fused map: hb x wb is its hc x wc.
 * Fused pixel (X, Y) of photo p, value v_l of level l:
 *   tile_value(l, x, y) = maps[first + owner(y)*kx + owner(x)][y - o_owner(y)][x - o_owner(x)]  with the cover of hc (halo_y) and
 *                         of wc (halo_x); 0.0f when that tile index is not in [0, T) or a table whose ky, kx are not the
 *                         cover's puts the local coordinate outside [0, th) x [0, tw): no element outside maps is read
 *   l == base:  v_l = tile_value(l, X, Y)
 *   otherwise   x = (X + 0.5)*ratio_x - 0.5  (float64, the product and the sum each rounded; ratio_x = (double)wc / (double)wb, one
 *               correctly rounded division, evaluated by the host), clamped to [0, wc - 1];  ix = floor(x), fx = (float)(x - ix),
 *               ix1 = min(ix + 1, wc - 1);  y, iy, fy, iy1 likewise from Y, ratio_y = (double)hc / (double)hb and hc;  each of the
 *               four taps is tile_value at its OWN owner tile (taps may straddle a core border)
 *               top = tap(ix, iy)*(1 - fx) + tap(ix1, iy)*fx, bot = tap(ix, iy1)*(1 - fx) + tap(ix1, iy1)*fx
 *               v_l = top*(1 - fy) + bot*fy                                               (float32, no fma)
 *   fuse 0 (max):   out = fmaxf(...fmaxf(fmaxf(v_0, v_1), v_2)...)                        (listed order)
 *   fuse 1 (mean):  out = ((v_0 + v_1) + ...) / (float)levels                             (float32, listed order)
 *   out[offset + Y*wb + X] = out                                                          (offset in ELEMENTS of the packed f32 buffer)
 * A photo whose map does not lie inside [0, out_elems), whose levels do not lie inside the level table, or whose hb, wb, levels
 * or base are out of range is skipped (nothing of it is written).  max_pixels: the largest hb*wb of the table (the launch is
 * sized by it; pixels beyond it are not written).  MR_ERR_ARG, nothing written: a null pointer with P > 0, T, L or P < 0, th or
 * tw < 1, a halo < 0 or th <= 2*halo_y or tw <= 2*halo_x, T*th*tw >= 2^31, max_pixels < 1 or >= 2^31, out_elems < 0, P > 65535, fuse outside {0, 1};
 * MR_ERR_DTYPE: another dtype.  P == 0 returns MR_OK without a launch. */
#define MR_TILE_FUSE_MAX 0
#define MR_TILE_FUSE_MEAN 1
typedef struct mr_tile_desc {
  int image;                    /* index into the mr_crop_image table */
  int x0, y0;                   /* canvas coordinates of the tile's first pixel */
  int wc, hc;                   /* the canvas: columns and rows of the resized photo */
  int reserved;                 /* 0 (keeps the doubles 8-byte aligned) */
  double scale_x, scale_y;      /* cv2.resize scales: 1. / ((double)wc / w), 1. / ((double)hc / h) */
} mr_tile_desc;
typedef struct mr_stitch_level {
  int hc, wc;                   /* the level's canvas: rows and columns */
  int ky, kx;                   /* its tile grid (the cover's K of hc and of wc) */
  int first;                    /* index of its tile (0, 0) in the tile maps */
  int reserved;                 /* 0 (keeps the doubles 8-byte aligned) */
  double ratio_x, ratio_y;      /* (double)wc / (double)wb and (double)hc / (double)hb of its photo; not read for the base level */
} mr_stitch_level;
typedef struct mr_stitch_photo {
  long long offset;             /* first element of the photo's fused map in the packed f32 output */
  int hb, wb;                   /* rows and columns of the fused map: the base level's canvas */
  int levels, first_level;      /* its entries of the level table: first_level .. first_level + levels - 1 */
  int base;                     /* which of them (0 .. levels - 1) is the base level */
  int reserved;                 /* 0 */
} mr_stitch_photo;
int mr_sizeof_tile_desc(void);
int mr_sizeof_stitch_level(void);
int mr_sizeof_stitch_photo(void);
int mr_tile_sample(const unsigned char* src, const void* images /* [I] */, int I, const void* tiles /* [T] */, int T, int th,
                   int tw, double mean0, double mean1, double mean2, float* dst /* [T][3][th][tw] */, hipStream_t stream);
int mr_tile_stitch(int dtype, const void* maps /* [T][th][tw] */, int T, int th, int tw, int halo_y, int halo_x,
                   const void* levels /* [L] */, int L, const void* photos /* [P] */, int P, long long max_pixels, int fuse,
                   float* out, long long out_elems, hipStream_t stream);

/* ---- Synthetic text (csrc/synth_text.hip): labelled word crops and scenes rendered on the device, from glyph atlases and tables
 * the host plans in float64 (megreader_amd/data/synth_text.py).  One launch renders N canvases of H x W pixels: a background, the
 * words ("items") of the canvas warped onto it with a drop shadow, a 5 x 5 separable blur, noise, and the quantised result as
 * uint8 HWC (B, G, R like a decoded photo) and / or as the recogniser's normalised f32 planes.
 *
 * Tables.  All live in memory the device reads.  `base` is the address every byte offset below is relative to (offsets may be
 * negative: an atlas or a photo resident in another allocation).
 *   fonts [F]: a font is a uint8 coverage image ("atlas") of gh rows and aw columns, row j at base + atlas_off + j*pitch, and the
 *     pairs glyphs[2*(glyph_first + id)] = x0, glyphs[2*(glyph_first + id) + 1] = w for class ids 0 <= id < n_classes: the glyph's
 *     first column in the atlas and its advance box (bearings are inside the box).  `glyphs` holds G pairs in all.  A pair is
 *     VALID when 0 <= glyph_first + id < G, x0 >= 0, 0 < w <= MR_SYNTH_MAX_GLYPH_W and x0 + w <= aw; every other pair, w = 0
 *     (a class without a glyph) included, and every id outside [0, n_classes), counts as w = 0.
 *   items [I]: a word: its canvas, its font, n_glyphs <= MR_SYNTH_MAX_GLYPHS class ids, the projective map h[9] canvas -> line
 *     (float64, row major), the integer box [x0, x1) x [y0, y1) of canvas pixels outside which it contributes nothing, the colours
 *     fg[3] and shadow[3] (float, in the order of the output channels), shadow_alpha, and the shadow's offset (shadow_dx,
 *     shadow_dy) in line pixels.  An item whose font is outside [0, F), whose font has gh < 1, whose n_glyphs is outside
 *     [0, MR_SYNTH_MAX_GLYPHS] or whose `canvas` is not the index of the canvas that lists it contributes nothing.
 *   canvases [N]: items first_item .. first_item + n_items - 1 in table order (n_items <= MR_SYNTH_MAX_ITEMS: a larger count is
 *     cut to it, a negative one is 0; indices outside [0, I) name no item); the background (photo == 0: two colours bg0, bg1 and a gradient gx, gy, g0; photo != 0: a resident uint8 HWC
 *     photo of at least H rows and W columns, row y at base + photo_off + y*photo_pitch); blur != 0: the taps w0, w1, w2 of the
 *     symmetric kernel (w2, w1, w0, w1, w2); the noise amplitude and a 32-bit seed (the int's bits).
 *
 * The virtual line image of an item.  start[0] = 0, start[g + 1] = start[g] + w of glyph g (0 for a pair that is not valid); the
 * line has Lw = start[n_glyphs] columns and gh rows.  Column i, 0 <= i < Lw, belongs to the one glyph g with
 * start[g] <= i < start[g + 1], and L(i, j) = atlas[j][x0[g] + i - start[g]]; L is 0 outside [0, Lw) x [0, gh).  Only bytes
 * atlas[j][k], 0 <= j < gh, 0 <= k < aw, are ever read, whatever the tables hold.
 *
 * Canvas pixel (x, y), channel c.  Every product and sum is rounded on its own, no fma, in the precision named; fmin / fmax
 * return the other operand for a NaN.
 *   comp(x, y), float32 unless marked:
 *     background: t = fminf(fmaxf(gx*(x + 0.5f) + gy*(y + 0.5f) + g0, 0), 1)           (left to right)
 *                 col[c] = bg0[c] + (bg1[c] - bg0[c]) * t;      with a photo: col[c] = (float)photo[y][x][c]
 *     for each item of the canvas in table order with x0 <= x < x1 and y0 <= y < y1:
 *       float64, left to right as mr_quad_crop:  px = x + 0.5, py = y + 0.5
 *         X = h[0]*px + h[1]*py + h[2], Y = h[3]*px + h[4]*py + h[5], D = h[6]*px + h[7]*py + h[8]
 *         u = X / D - 0.5, v = Y / D - 0.5
 *       cov(u, v): 0 when D <= 0 (or NaN) or not (-1 < u < Lw and -1 < v < gh) (which a NaN or an infinity fails); otherwise
 *         iu = floor(u), fu = (float)(u - iu); iv = floor(v), fv = (float)(v - iv); the four taps L(iu, iv), L(iu + 1, iv),
 *         L(iu, iv + 1), L(iu + 1, iv + 1) as float and the float32 blend top, bot, val of mr_warp_normalize; cov = val / 255.f
 *       a = cov(u, v);  if shadow_alpha != 0: s = cov(u - shadow_dx, v - shadow_dy) (float64 differences), ts = s * shadow_alpha,
 *         col[c] = col[c]*(1.f - ts) + shadow[c]*ts.   Then col[c] = col[c]*(1.f - a) + fg[c]*a.
 *   blur != 0:  with xi = min(max(x + i, 0), W - 1), yj = min(max(y + j, 0), H - 1) and k[-2..2] = (w2, w1, w0, w1, w2):
 *       row(x, yj)[c] = k[-2]*comp(x-2, yj)[c] + k[-1]*comp(x-1, yj)[c] + k[0]*comp(x, yj)[c] + k[1]*comp(x+1, yj)[c] + k[2]*comp(x+2, yj)[c]
 *       col[c] = k[-2]*row(x, y-2)[c] + k[-1]*row(x, y-1)[c] + k[0]*row(x, y)[c] + k[1]*row(x, y+1)[c] + k[2]*row(x, y+2)[c]
 *     (each sum left to right, starting from its first product; the x +- i and y +- j above stand for the clamped xi, yj).
 *     blur == 0: col = comp(x, y).
 *   noise, uint32 arithmetic modulo 2^32:  k = (y*W + x)*3 + c;  r = seed + k * 0x9E3779B9;
 *       r ^= r >> 16;  r *= 0x7FEB352D;  r ^= r >> 15;  r *= 0x846CA68B;  r ^= r >> 16;                          ("lowbias32")
 *       col[c] = col[c] + noise_amp * ((float)(r >> 8) * 0x1p-24f - 0.5f)
 *   q[c] = fminf(fmaxf(floorf(col[c] + 0.5f), 0), 255)
 *   out_u8[n][y][x][c] = (unsigned char)q[c];   out_f32[n][c][y][x] = (float)((double)q[c] - mean[c]) / 255.f
 * The f32 output is the normalising store of mr_resize_normalize: bit-equal to mr_resize_normalize of out_u8 at identity scale.
 * Either output may be NULL (not both); every element of a given output is written.  A canvas's pixels are a function of its
 * own table entries alone: they do not depend on N, on the canvas's position in the call or on the launch geometry.
 *
 * One launch on `stream` (a workgroup per MR_SYNTH_TILE_H x MR_SYNTH_TILE_W tile of a canvas), no allocation, no
 * synchronisation; N == 0 returns MR_OK without a launch.  MR_ERR_ARG, nothing written: H or W < 1, N, F, G or I < 0, more than
 * INT_MAX tiles, a NULL table that has elements (canvases; items when I > 0; fonts when F > 0; glyphs when G > 0), both outputs
 * NULL.  When `canvases` / `items` / `fonts` are pinned host memory (and `stream` is not being captured) the entry point also
 * refuses, before the launch, a canvas
 * whose items are not inside [0, I) or more than MR_SYNTH_MAX_ITEMS, an item whose n_glyphs, font or canvas is out of range or
 * not listed by its canvas, and a font whose glyph pairs are not inside [0, G).  Tables it cannot read are the kernel's to
 * guard: every loop of the kernel is bounded by the limits above whatever the tables hold. */
#define MR_SYNTH_MAX_GLYPHS 32
#define MR_SYNTH_MAX_ITEMS 32
#define MR_SYNTH_MAX_GLYPH_W 65536
#define MR_SYNTH_TILE_H 16
#define MR_SYNTH_TILE_W 64
typedef struct mr_synth_font {
  long long atlas_off;          /* byte offset of atlas row 0 from base */
  int pitch;                    /* bytes per atlas row (>= aw) */
  int gh, aw;                   /* rows and columns of the atlas */
  int glyph_first, n_classes;   /* this font's pairs are glyphs[2*glyph_first .. 2*(glyph_first + n_classes)) */
  int reserved;                 /* 0 (pads the entry to 32 bytes) */
} mr_synth_font;
typedef struct mr_synth_item {
  int canvas, font, n_glyphs;
  int reserved;                 /* 0 */
  int x0, x1, y0, y1;           /* the item's box of canvas pixels */
  float fg[3], shadow[3];
  float shadow_alpha;
  float reserved1;              /* 0 (keeps the doubles 8-byte aligned) */
  double shadow_dx, shadow_dy;  /* line pixels */
  double h[9];                  /* canvas -> line, row major, projective */
  int glyph[32];                /* class ids (MR_SYNTH_MAX_GLYPHS entries) */
} mr_synth_item;
typedef struct mr_synth_canvas {
  int first_item, n_items;
  int photo;                    /* 0: gradient background, otherwise the photo at photo_off */
  int blur;                     /* 0: no blur */
  float bg0[3], bg1[3];
  float gx, gy, g0;
  float w0, w1, w2;             /* blur taps: (w2, w1, w0, w1, w2) */
  float noise_amp;
  int seed;                     /* the 32 bits of the noise seed */
  long long photo_off;          /* byte offset of the photo's first pixel from base */
  int photo_pitch;              /* bytes per photo row (>= 3 * W) */
  int reserved;                 /* 0 */
} mr_synth_canvas;
int mr_sizeof_synth_font(void);
int mr_sizeof_synth_item(void);
int mr_sizeof_synth_canvas(void);
int mr_synth_render(const unsigned char* base, const void* fonts /* [F] */, int F, const int* glyphs /* [G][2] */, int G,
                    const void* items /* [I] */, int I, const void* canvases /* [N] */, int N, int H, int W, double mean0,
                    double mean1, double mean2, unsigned char* out_u8 /* [N][H][W][3] or NULL */,
                    float* out_f32 /* [N][3][H][W] or NULL */, hipStream_t stream);

/* ---- Recognition augmentation (csrc/rec_augment.hip): the recogniser's training augmentation -- geometric jitter, a wavy
 * baseline, a colour map, a 5 x 5 blur, noise, pixelation and erased rectangles, per sample -- in ONE bilinear pass from the
 * resident uint8 HWC photos (stored crops, or scenes that hold the words) to the recogniser's normalised f32 planes.  The host
 * plans every sample in float64 from shapes alone (megreader_amd/data/recognition_augment.py); the device reads each source
 * pixel once.  `images` is the photo table of mr_quad_crop (`offset` relative to src, may be negative).
 *
 * The call writes the whole rows dst[row] of its M descriptors and NOTHING else: rows that no descriptor names keep their bytes,
 * so a pipeline runs its plain kernel over the batch and this one over the augmented rows, and the other samples keep their bits.
 *
 * Every product and sum is rounded on its own, no fma, in the precision named; fmin / fmax (min / max below) return the other
 * operand for a NaN.  With Wv = min(max(dst_w, 0), W), canvas pixel (u, v) of a descriptor, u < Wv:
 *   comp(u, v):
 *     q = max(quant, 1);  bu = (u / q)*q, bv = (v / q)*q                                  (integer division)
 *     U = (double)bu + 0.5*(double)q, V = (double)bv + 0.5*(double)q                      (float64 from here)
 *     t = U*8.0 / (double)Wv;  j = (int)min(max(floor(t), 0), 7);  f = t - (double)j
 *     U' = U + ((double)dx[j] + ((double)dx[j+1] - (double)dx[j])*f),  V' = V + ((double)dy[j] + ((double)dy[j+1] - (double)dy[j])*f)
 *     cx = U'*sx - 0.5, cy = V'*sy - 0.5                                                  (cv2.resize's sampling point, displaced)
 *     X = g[0]*cx + g[1]*cy + g[2], Y = g[3]*cx + g[4]*cy + g[5], D = g[6]*cx + g[7]*cy + g[8]     (left to right, as mr_quad_crop)
 *     D <= 0 (or NaN): val = 0.  Otherwise px = min(max(X / D, cu0), cu1), py = min(max(Y / D, cv0), cv1), and (px, py) goes
 *     through h[9] as mr_quad_crop's (cx, cy) does: X2 = h[0]*px + h[1]*py + h[2], Y2, D2 likewise, x = X2 / D2, y = Y2 / D2;
 *     D2 <= 0 (or NaN), or x or y not finite: val = 0; otherwise floor, (float) fractions, the four taps (0 outside
 *     [0, w) x [0, h) of the photo) and the float32 blend top, bot, val of mr_warp_normalize
 *     col[c] = fminf(fmaxf(m[3c]*val[0] + m[3c+1]*val[1] + m[3c+2]*val[2] + b[c], 0), 255)     (float32, left to right)
 *   blur != 0:  col[c] = the sum over j = -2..2 (outer) and i = -2..2 (inner), left to right starting from its first product, of
 *                        k[(j+2)*5 + (i+2)] * comp(min(max(u + i, 0), Wv - 1), min(max(v + j, 0), H - 1))[c]              (float32)
 *   blur == 0:  col = comp(u, v)
 *   erase:  for e = 0 .. min(max(n_erase, 0), MR_AUG_MAX_ERASE) - 1 in order, with (x0, x1, y0, y1) = erase[4e .. 4e + 3]:
 *           x0 <= u < x1 and y0 <= v < y1  ->  col[c] = erase_col[3e + c]
 *   noise:  the rule of mr_synth_render, uint32 arithmetic modulo 2^32:  kk = (v*W + u)*3 + c;  r = lowbias32(seed + kk * 0x9E3779B9)
 *           col[c] = col[c] + noise_amp * ((float)(r >> 8) * 0x1p-24f - 0.5f);  col[c] = fminf(fmaxf(col[c], 0), 255)
 *   dst[row][c][v][u] = (float)((double)col[c] - mean[c]) / 255.f                         (as mr_resize_normalize ends)
 * Columns u >= Wv get the normalised zero pixel, and so does every pixel of a descriptor whose `image` is not in [0, I).  A
 * descriptor whose `row` is not in [0, N) writes nothing.  Only bytes src[offset + r*pitch + 3*k + c], 0 <= r < h, 0 <= k < w, of
 * photos in the table are read, whatever the tables hold, and every loop is bounded by the limits above.  A row's pixels are a
 * function of its own descriptor alone: not of M, of the descriptor's position in the call or of the launch geometry.
 *
 * Consequence: the IDENTITY descriptor -- g = identity, dx = dy = 0, m = identity, b = 0, blur = 0, n_erase = 0, noise_amp = 0,
 * quant = 1, cu0 = cv0 = 0 -- writes the row that mr_quad_crop writes for the mr_crop_desc with the same image, dst_w, sx, sy,
 * cu1, cv1 and h, bit for bit (X = cx, D = 1 and col = val are exact).
 *
 * One launch on `stream` (a workgroup per MR_SYNTH_TILE_H x MR_SYNTH_TILE_W tile of a descriptor's canvas; comp is evaluated once
 * per pixel of the tile and its halo of 2), no allocation on the device, no synchronisation; capturable.  M == 0 returns MR_OK
 * without a launch.  MR_ERR_ARG, nothing written: a NULL src, images, descs or dst with M > 0, I, M or N < 0, H or W < 1, more
 * than INT_MAX tiles.  When `descs` is pinned host memory and `stream` is not being captured the entry point also refuses, before
 * the launch, a `row` that two descriptors name, a `row` outside [0, N), an `image` outside [0, I), an `n_erase` outside
 * [0, MR_AUG_MAX_ERASE] and a `dst_w` outside [1, W].  A table it cannot read is the kernel's to guard, as above; two descriptors
 * of such a table that name one row leave that row as either of them. */
#define MR_AUG_KNOTS 9
#define MR_AUG_MAX_ERASE 4
typedef struct mr_aug_desc {
  int image;                    /* index into the mr_crop_image table */
  int row;                      /* destination row of dst */
  int dst_w;                    /* valid canvas columns; the rest is the zero canvas */
  int quant;                    /* pixelation block in canvas pixels; 1 (or less) = off */
  int blur;                     /* 0: k is not applied */
  int n_erase;                  /* rectangles of `erase` in use, 0 .. MR_AUG_MAX_ERASE */
  int seed;                     /* the 32 bits of the noise seed */
  int reserved;                 /* 0 (keeps the doubles 8-byte aligned) */
  double sx, sy;                /* cv2.resize scales of the frame, as mr_crop_desc */
  double cu0, cu1, cv0, cv1;    /* the frame coordinate is clamped to [cu0, cu1] x [cv0, cv1] */
  double g[9];                  /* jitter: output frame -> source frame, row major, projective */
  double h[9];                  /* frame -> photo, row major, projective: identity for a stored crop, mr_crop_desc.h for a quad crop */
  float dx[9], dy[9];           /* displacement of the sampling point in canvas pixels at MR_AUG_KNOTS knots over [0, dst_w] */
  float m[9], b[3];             /* colour: col = m * val + b, row major */
  float k[25];                  /* 5 x 5 blur kernel, row major (rows are v) */
  float noise_amp;
  int erase[16];                /* [MR_AUG_MAX_ERASE][4]: x0, x1, y0, y1 of [x0, x1) x [y0, y1) in canvas pixels */
  float erase_col[12];          /* [MR_AUG_MAX_ERASE][3]: the fill colour of each rectangle */
} mr_aug_desc;
int mr_sizeof_aug_desc(void);
int mr_rec_augment(const unsigned char* src, const void* images /* [I] mr_crop_image */, int I,
                   const void* descs /* [M] mr_aug_desc */, int M, int N, int H, int W,
                   double mean0, double mean1, double mean2, float* dst /* [N][3][H][W] */, hipStream_t stream);

/* ---- Lexicon-constrained reading (csrc/lexicon.hip): the nearest lexicon word of every predicted id sequence, the rule of the
 * recognition benchmarks that are reported with lexicons (50 words per image, 1 k per set, "full"), and the membership test of
 * structure/measurers/sequence_recognition_measurer.py:59-64 (`in_lexicon`: distance 0).
 *   preds: i32 [N, S], S <= MR_SEQ_MEASURE_MAX.  Row n's sequence is its S entries with `blank` and `unknown` dropped, then mapped
 *     through `fold` (nullable; id -> canonical id, C entries) -- exactly how mr_seq_measure reads a row.  pred_len[n] = m, the
 *     number of symbols left.
 *   word l = lex_sym[lex_off[l] .. lex_off[l+1]), 0..MR_LEXICON_MAX_WORD symbols, already folded by the host, no blank.  It may
 *     hold `unknown`, which matches nothing.  lex_off lives on the device, so the entry point cannot check the word lengths without
 *     a synchronising copy: the caller guarantees them (megreader_amd/ops/lexicon.py raises on a longer word); the kernel reads at
 *     most MR_LEXICON_MAX_WORD symbols of a word whatever lex_off says.
 *   span: nullable i32 [N, 2]: row n's candidates are the words [span[n][0], span[n][1]) (clamped to [0, L]); NULL: [0, L).
 *     Per-image lexicons laid end to end and one shared lexicon go through the same entry point.
 *   C: number of classes.  An id outside [0, C) on either side matches nothing and indexes no table.
 *   best_dist[n] = the smallest Levenshtein distance between row n and a candidate, best_index[n] = the lowest word index that
 *     reaches it; -1 / -1 for an empty candidate range.  All three outputs are written for every row; nothing has to be zeroed.
 * Rows of m <= 64 symbols run the bit-parallel recurrence (Myers 1999 / Hyyro) with the prediction as the pattern, one thread per
 * candidate word, the match masks of the prediction in LDS: a table of C entries up to C = 8192, the <= 64 distinct symbols of the
 * prediction beyond.  Longer rows swap the roles (the word is the pattern) in the same launch: slow, exact.  The per-row minimum
 * of (distance << 32 | index) is taken with 64-bit atomics in a key buffer the library owns per device (8 bytes per row, grown
 * outside stream capture only: under capture, N must not exceed the largest N of an earlier call on that device); calls on one
 * device must therefore be stream-ordered with each other.  Deterministic.  N == 0 returns MR_OK without a launch; S == 0 reads
 * no element of preds.  MR_ERR_ARG, nothing written: S above the cap, C < 2, a negative size. */
#define MR_LEXICON_MAX_WORD 64      /* symbols per lexicon word */
int mr_lexicon_nearest(const int* preds, int S, int N, int blank, int unknown, const int* fold,
                       const int* lex_sym, const int* lex_off, int L, const int* span, int C,
                       int* best_index, int* best_dist, int* pred_len, hipStream_t stream);

/* ---- Lexicon transcription by CTC likelihood (csrc/lexicon.hip): the lexicon-based transcription of the CRNN paper (Shi et al.,
 * "An End-to-End Trainable Neural Network for Image-based Sequence Recognition", section 2.3.2): l* = argmax over the lexicon words
 * l within edit distance delta of the greedy string of p(l | y), the CTC probability of the word summed over all alignments.
 *   Posterior.  Row n has T columns and C classes; y[t, c] is read from pred + n*sn + c*sc + t*st (element strides; dtype
 *     MR_DTYPE_F32 or MR_DTYPE_BF16, converted to f32 on load).  With log_probs == 0 (probabilities, the eval head's softmax)
 *     lp[t, c] = the f32 nearest to log y[t, c] (the log taken in f64 and rounded once; y = 0 gives -inf); otherwise y[t, c]
 *     itself -- logs rounded that way give the same scores bit for bit as the probabilities they were taken from.  The classes are the folded ones: a caller whose charset
 *     folds case sums the posterior over each fold class first (megreader_amd/ops/lexicon.py).
 *   Words, span, C, blank, unknown, fold: as mr_lexicon_nearest; 0 <= blank < C.
 *   Score.  score(n, l) = log of the sum, over all paths of T classes that collapse to the word (merge repeats, then drop blanks),
 *     of the product of y[t, path_t], by the alpha recursion over the blank-extended word e (e[2i] = blank, e[2i+1] = symbol i,
 *     2K + 1 positions) in f32 logs:
 *       alpha_0(0) = lp[0, blank], alpha_0(1) = lp[0, e[1]], every other position -inf
 *       alpha_t(s) = lp[t, e[s]] + lse(alpha_{t-1}(s), alpha_{t-1}(s-1), alpha_{t-1}(s-2) if s is odd and e[s] != e[s-2])
 *       score = lse(alpha_{T-1}(2K), alpha_{T-1}(2K-1));  K = 0: alpha_{T-1}(0), the sum over t of lp[t, blank]
 *     lse(a, b, ..) = m + log(exp(a - m) + exp(b - m) + ..) with m the greatest term, and -inf when every term is -inf: a zero
 *     probability flows through without a NaN.  A word that cannot fit -- K + (number of adjacent equal symbol pairs) > T -- and a
 *     word that holds `unknown` or an id outside [0, C) score -inf without a recursion.  score(n, l) is a function of row n's
 *     values and the word's symbols alone, bit for bit: not of the word's index, the span, max_distance, N or the launch.
 *   Candidates.  The words of row n's span; with max_distance >= 0 only those whose Levenshtein distance to the row of `preds` is
 *     <= max_distance.  preds: i32 [N, S], the greedy ids (mr_ctc_greedy_decode on the same pred; S = T), read exactly as
 *     mr_lexicon_nearest reads a row: blank / unknown dropped, then `fold`.  max_distance < 0: every word of the span, and no
 *     distance is taken for the selection.
 *   Outputs, all written for every row, nothing to be zeroed: best_index[n] the candidate with the greatest score, the lowest
 *     index among bit-equal scores; best_score[n] (f32) its score; best_dist[n] its edit distance to the row; -1 / -inf / -1 when no
 *     candidate has a finite score.  pred_len[n] as mr_lexicon_nearest.  n_cand[n] the number of candidates after the distance
 *     filter, whether or not their score is finite.  all_scores (nullable f32 [N, L]): score(n, l) of every candidate, -inf for
 *     every other word.
 * Lane i of a word's lanes holds symbol i and the two positions 2i, 2i+1, one value crosses lanes per column; a wave scores four
 * words of at most 15 symbols side by side, longer ones one at a time.  A row's [C, T] log-probabilities are staged in LDS when
 * C * (T | 1) <= 8192 and read from global memory otherwise.  The per-row maximum is taken with 64-bit atomics in the key buffer of mr_lexicon_nearest, so the same rules hold: calls of either entry
 * point on one device are stream-ordered with each other, and under stream capture N must not exceed the largest N of an earlier
 * call on that device.  Deterministic.  N == 0 returns MR_OK without a launch.  MR_ERR_ARG, nothing written: T < 1, S above the
 * cap, C < 2, blank outside [0, C), a negative size; MR_ERR_DTYPE: another dtype code. */
int mr_lexicon_transcribe(int dtype, const void* pred, long long sn, long long sc, long long st, int T, int log_probs,
                          const int* preds, int S, int N, int blank, int unknown, const int* fold,
                          const int* lex_sym, const int* lex_off, int L, const int* span, int C, int max_distance,
                          int* best_index, float* best_score, int* best_dist, int* pred_len, int* n_cand,
                          float* all_scores, hipStream_t stream);

/* ---- CTC prefix beam search (csrc/ctc_beam.hip): the most probable STRINGS of a CTC posterior with their log-probabilities, where
 * mr_ctc_greedy_decode gives the most probable path (Graves; Hannun et al., "First-pass large vocabulary continuous speech
 * recognition using bi-directional recurrent DNNs", Algorithm 1, without the language model).  Two columns `blank 0.6 / A 0.4`:
 * the best path spells "" (0.36), the string "A" has probability 0.64.
 *   Posterior.  Row n has T columns and C classes; lp[t, c] is defined exactly as for mr_lexicon_transcribe: y[t, c] read from
 *     pred + n*sn + c*sc + t*st (element strides; MR_DTYPE_F32 or MR_DTYPE_BF16, converted to f32 on load); with log_probs == 0
 *     lp[t, c] = the f32 nearest to log y[t, c] (the log taken in f64 and rounded once; y = 0 gives -inf), otherwise y[t, c] itself.
 *   Parameters.  beam B in 1..MR_CTC_BEAM_MAX; nbest K in 1..B; top_classes Kc in 1..MR_CTC_BEAM_TOP_MAX; blank in [0, C);
 *     unknown: any int, outside [0, C) means "there is none".
 *   Hypotheses.  A hypothesis is a prefix: a tuple of class ids with neither blank nor `unknown`.  It carries two f32 log masses:
 *     pb, the alignments that end in blank, and pnb, those that end in its last symbol; total = lse(pb, pnb).  The start state is
 *     the empty prefix with pb = 0, pnb = -inf.  lse(a, b) = m + log(exp(a - m) + exp(b - m)) with m the greater term, and -inf
 *     when both are -inf: a zero probability flows through without a NaN.  `+=` below is lse; every right-hand side is the value
 *     from before column t.  Per column t:
 *       1. Symbols of the column: the min(Kc, eligible) classes with the greatest lp[t, c] among c != blank, c != unknown,
 *          lp[t, c] > -inf; among bit-equal values the lower id wins.  `unknown` is never emitted and its mass is lost, as in
 *          mr_lexicon_transcribe, where a word that holds `unknown` matches nothing.
 *       2. Stay.  For every prefix p of the beam: pb'(p) += total(p) + lp[t, blank]; if p is not empty, pnb'(p) += pnb(p) +
 *          lp[t, last(p)] -- always, whether or not last(p) is among the column's symbols (it is read from the posterior itself).
 *       3. Extend.  For every prefix p and column symbol c: pnb'(p + c) += (pb(p) if c == last(p) else total(p)) + lp[t, c].
 *       4. Merge.  Contributions to the same prefix are added, and sameness is by CONTENT: an extension p + c that spells a prefix
 *          already in the beam joins that prefix's stay masses, also when p had left the beam and came back meanwhile.
 *       5. Keep.  The B prefixes with the greatest total survive; a prefix whose total is -inf is dropped, so the beam may hold
 *          fewer than B, or none.
 *   Outputs.  After the last column the K greatest by total, in descending order: ids i32 [N, K, T] blank padded, lengths i32
 *     [N, K], scores f32 [N, K] (the totals), count i32 [N] = the number of hypotheses returned, 0..K.  Slots past count get length
 *     0, score -inf and all blank; the empty string is a legitimate hypothesis (length 0, a finite score).  Every output is written
 *     for every row, nothing has to be zeroed.  The order among bit-equal totals is unspecified (step 5 and the output), the
 *     result is deterministic all the same: a function of the row's values and the parameters alone, bit for bit, not of N, the
 *     row's position or the launch.
 *   What follows.  With Kc >= the eligible classes and B >= the number of distinct labelings nothing is pruned and the scores are
 *     the exact log p(string | y) of EVERY string (to f32 rounding); otherwise every score is a LOWER BOUND of its string's
 *     log p(string | y): the pruned alignments are missing.
 *   Workspace.  The caller passes ws of at least mr_ctc_beam_ws_bytes(N, T, beam, top_classes) bytes, 8-byte aligned, contents
 *     arbitrary: the column lists (id, lp) [N, T, Kc] and, per row, the trie of its prefixes (an open-addressing table keyed by the
 *     exact pair (parent node, symbol), 2 * T * beam + 64 entries of 8 bytes).  The query is host only, works without a GPU and
 *     returns 0 for arguments the entry point refuses -- a workspace above INT_MAX bytes among them: split the batch.  The call
 *     allocates nothing, does not synchronise and does no host work that depends on device data: two launches on `stream`
 *     (one wave per column, then one wave per row), capturable in a graph.
 * N == 0 returns MR_OK without a launch.  MR_ERR_ARG, nothing written: T < 1 or above MR_SEQ_MEASURE_MAX, C < 2, blank outside
 * [0, C), beam / nbest / top_classes out of range, a workspace that is too small, misaligned or null, a negative size;
 * MR_ERR_DTYPE: another dtype code. */
#define MR_CTC_BEAM_MAX 64          /* hypotheses kept per row */
#define MR_CTC_BEAM_TOP_MAX 64      /* symbols considered per column */
int mr_ctc_beam_ws_bytes(int N, int T, int beam, int top_classes);  /* host only */
int mr_ctc_beam_search(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T,
                       int log_probs, int blank, int unknown, int beam, int nbest, int top_classes,
                       int* ids, int* lengths, float* scores, int* count, void* ws, long long ws_bytes, hipStream_t stream);

/* ---- CTC prefix beam search with a character n-gram language model (csrc/ctc_beam.hip): Hannun et al., Algorithm 1, WITH the
 * language model.  The strings are ranked by log p_ctc(string | y) + alpha * log p_lm(string) + beta * |string|, so that a reader
 * without a closed lexicon prefers "the" to "tbe".  Posterior, parameters, hypotheses, workspace (mr_ctc_beam_ws_bytes) and the
 * two launches are those of mr_ctc_beam_search; what is added:
 *   Model.  A backoff n-gram model (ARPA's) over the class ids, of order 1..MR_NGRAM_ORDER_MAX, as a finite automaton with `states`
 *     states: one per listed context shorter than the order, state 0 the empty context.  For a state s and a class c
 *       g(c | s) = arc_lp(s, c) if the arc (s, c) is listed, else bow[s] + g(c | backoff[s]);  no arc at state 0: -inf
 *     accumulated in f32 in that order: acc = 0, acc += bow[s] for every state backed off through, g = acc + arc_lp.  The state
 *     after c is arc_next of the arc that was found: the longest suffix of context + c that is a state.
 *     Arcs: an open-addressing table of `slots` entries in three arrays, lm_keys u64 (key (s << 32) | (c + 1); 0 = empty),
 *     lm_arc_lp f32, lm_arc_next i32.  Hash and probing, in 32-bit unsigned arithmetic (host and kernel follow this one rule):
 *       h = (s * 0x9E3779B1) ^ ((c + 1) * 0x85EBCA6B);  h = (h ^ (h >> 15)) % slots;  then h, h + 1, .. (wrapping at slots)
 *     An arc lies within the first max_probe slots of its sequence with no empty slot before it (max_probe = the longest probe
 *     sequence of the table as built, >= 1): a lookup that meets an empty slot, or has read max_probe slots, is a miss.
 *     Per state: lm_bow f32, lm_backoff i32 (the state of the context without its first symbol, -1 for state 0), lm_end_lp f32
 *     (g(</s> | s) backed off to the end on the host; 0 for a model without </s>).  The caller guarantees: every lm_arc_next and
 *     every lm_backoff but that of state 0 lies in [0, states), backoff chains reach state 0 within order - 1 steps, state 0 lists
 *     every class that may be a symbol (neither blank nor `unknown`), all values are finite.  (megreader_amd/ops/language_model.py
 *     builds and checks such an image.)  The kernel stops a chain at a state outside [0, states) as at a miss in state 0.
 *   Rule.  Every hypothesis also carries a model state and an f32 sum lm(p); the empty prefix starts with (start_state, 0).
 *       lm(p + c) = lm(p) + (alpha * g(c | state(p)) + beta),  state(p + c) = the state after c
 *     every operation rounded to f32 on its own (no fused multiply-add).  Both are functions of the string alone, so an extension
 *     that merges into a stay (step 4) agrees with it and a prefix that re-enters the beam gets the same values back.  pb, pnb and
 *     total stay the pure CTC masses: steps 1 to 4 are those of mr_ctc_beam_search bit for bit, and step 1 still picks the
 *     column's symbols by lp alone.  An extension whose g is -inf is dropped.
 *       5. Keep.  The B prefixes with the greatest total + lm survive (one f32 addition; -inf is dropped).
 *     After the last column, with end != 0, lm(p) += alpha * lm_end_lp[state(p)] for every survivor, and the K greatest by
 *     total + lm are returned in descending order.
 *   Outputs.  ids, lengths, count as mr_ctc_beam_search; scores f32 [N, K] = total + lm, the ranked value; ctc_scores f32 [N, K] =
 *     total, still a lower bound of log p(string | y) and exact when nothing is pruned; lm_scores f32 [N, K] = lm.  Slots past
 *     count get -inf in all three.  With alpha == 0, beta == 0 and end == 0 ids, lengths, count and ctc_scores are those of
 *     mr_ctc_beam_search and lm_scores is 0.  Deterministic and row-independent as mr_ctc_beam_search; the model arrays are only read.
 * One lookup per extension (p, j), by the lanes that build the extension keys: at most `order` levels of at most max_probe probes.
 * N == 0 returns MR_OK without a launch.  MR_ERR_ARG, nothing written: everything mr_ctc_beam_search refuses; a null model
 * pointer; order outside 1..MR_NGRAM_ORDER_MAX; states < 1; slots < 1; max_probe < 1; start_state outside [0, states); alpha or
 * beta not finite.  MR_ERR_DTYPE: another dtype code. */
#define MR_NGRAM_ORDER_MAX 8        /* symbols per n-gram */
int mr_ctc_beam_search_lm(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T,
                          int log_probs, int blank, int unknown, int beam, int nbest, int top_classes,
                          const unsigned long long* lm_keys, const float* lm_arc_lp, const int* lm_arc_next,
                          const float* lm_bow, const int* lm_backoff, const float* lm_end_lp, int states, int slots,
                          int max_probe, int start_state, int order, float alpha, float beta, int end,
                          int* ids, int* lengths, float* scores, float* ctc_scores, float* lm_scores, int* count,
                          void* ws, long long ws_bytes, hipStream_t stream);

/* ---- Forced CTC alignment (csrc/ctc_align.hip): WHERE the symbols of a given string lie in a CTC posterior and how probable each
 * is there -- the single most probable alignment of the string (Viterbi), where mr_lexicon_transcribe sums over all of them.  It
 * answers what neither a lexicon word nor a beam hypothesis can: which columns carry which character (character boxes, per-
 * character confidence).
 *   Posterior.  Row n has T columns and C classes; lp[t, c] is defined exactly as for mr_lexicon_transcribe: y[t, c] read from
 *     pred + n*sn + c*sc + t*st (element strides; MR_DTYPE_F32 or MR_DTYPE_BF16, converted to f32 on load); with log_probs == 0
 *     lp[t, c] = the f32 nearest to log y[t, c] (the log taken in f64 and rounded once; y = 0 gives -inf), otherwise y[t, c] itself.
 *   Target.  targets: i32 [N, S], S in 0..MR_CTC_ALIGN_MAX_SYMBOLS; target_len: i32 [N], on the device, not nullable.  Row n's
 *     string is targets[n, 0 .. K) with K = target_len[n]; entries past K are not read.  The classes are taken as given (a caller
 *     whose charset folds case folds the posterior first, as megreader_amd/ops/lexicon.py does).  The row is UNALIGNABLE when K is
 *     outside [0, S], when a symbol equals `blank` or `unknown` or lies outside [0, C), or when the string cannot fit:
 *     K + (number of adjacent equal symbol pairs) > T.
 *   Recursion, over the blank-extended string e (e[2i] = blank, e[2i+1] = symbol i, 2K + 1 positions), in f32:
 *       d_0(0) = lp[0, blank], d_0(1) = lp[0, e[1]], every other position -inf
 *       d_t(s) = lp[t, e[s]] + max(d_{t-1}(s), d_{t-1}(s-1), d_{t-1}(s-2) if s is odd and e[s] != e[s-2])
 *     one f32 addition per cell, nothing fused; -inf flows through and no NaN appears.  The back-pointer of a cell is the
 *     predecessor that supplied the maximum; among equal candidates (all -inf included) the smallest step wins: s before s-1
 *     before s-2.  End position: 0 when K == 0; otherwise 2K if d_{T-1}(2K) >= d_{T-1}(2K-1), else 2K-1.  score[n] (f32) is d_{T-1}
 *     at the end position: the log-probability of the best alignment.
 *   Outputs, all written for every row, nothing to be zeroed.  pos i32 [N, T]: the position of every column on the path traced back
 *     from the end position.  For symbol i < K: begin[n, i] / end[n, i] (i32 [N, S]) the first column and one past the last column
 *     with pos == 2i + 1 (one run by construction, never empty); sym_lp[n, i] (f32 [N, S]) the sum of lp[t, symbol i] over those
 *     columns, added in ascending t starting from the first term; peak[n, i] (i32 [N, S]) the column of the run with the greatest
 *     lp, the lowest t among equal values.  Slots i >= K: begin = end = peak = -1, sym_lp = -inf.  An unalignable row, and a row
 *     whose score is -inf (the string is reachable only through zero-probability cells): score = -inf, every pos = -1, every slot
 *     filled as a slot past K.  A row's outputs are a function of that row's values and its target alone, bit for bit: not of N, S,
 *     the row's index or the launch.
 *   Workspace.  The caller passes ws of at least mr_ctc_align_ws_bytes(N, T, S) bytes, 8-byte aligned, contents arbitrary: the
 *     back-pointers, 4 bits per (column, symbol).  The query is host only, works without a GPU and returns 0 for arguments the entry
 *     point refuses and for a size above INT_MAX (split the batch).  The call allocates nothing, does not synchronise and does no
 *     host work that depends on device data: one launch on `stream`, capturable in a graph.
 * One wave per row.  Lane i holds symbol i and the positions 2i, 2i + 1 in registers (strings of 64 symbols and more: the symbols
 * i, i + 64, .. in further register slots), ONE value crosses lanes per column and slot; the blank after the last symbol sits with
 * "symbol" K.  Only the K + 1 classes the string names are read, and their logs taken, whatever C is.  A lane keeps its own
 * back-pointers (in LDS when the row's fit 16 KiB, else in the workspace) and later reads only those back, so the back-trace
 * loads whole columns ahead of the path it walks.
 * N == 0 returns MR_OK without a launch; S == 0 reads no element of targets.  MR_ERR_ARG, nothing written: S outside
 * 0..MR_CTC_ALIGN_MAX_SYMBOLS, T < 1 or above MR_SEQ_MEASURE_MAX, C < 2, blank outside [0, C), a negative size, a workspace that is
 * too small, misaligned or null; MR_ERR_DTYPE: another dtype code. */
#define MR_CTC_ALIGN_MAX_SYMBOLS 256  /* symbols per target string */
int mr_ctc_align_ws_bytes(int N, int T, int S);  /* host only */
int mr_ctc_align(int dtype, const void* pred, long long sn, long long sc, long long st, int N, int C, int T, int log_probs,
                 int blank, int unknown, const int* targets, int S, const int* target_len,
                 float* score, int* pos, int* begin, int* end, float* sym_lp, int* peak,
                 void* ws, long long ws_bytes, hipStream_t stream);

/* ---- Reading a 2D-CTC head with the 1-D readers (csrc/ctc2d_read.hip).  The eval output of a 2D-CTC head is classify [N, C, H, W]
 * (softmax over the classes) and mask [N, 1, H, W] (softmax over the heights).  The 2D-CTC recursion (ops/ctc_2d/csrc/cuda/
 * ctc2d_cuda_kernel.cu:125-175) sums alpha over all heights of the previous column before every step, so alpha summed over h obeys
 * the 1-D CTC recursion on q[n, c, w] = sum_h classify[n, c, h, w] * mask[n, 0, h, w]: the string probabilities of the 2-D head are
 * those of the 1-D posterior q, and mr_lexicon_transcribe, mr_ctc_beam_search and mr_ctc_align read it as they read any other.  (Two
 * differences from the training loss: it returns inf for an empty target, where the 1-D readers give the all-blank probability;
 * and it clamps every product at `tiny` before the log, which the eval tensors are not.)  With max for sum, mr_ctc_greedy_decode of
 * the result is the 2-D greedy rule of mr_ctc2d_greedy_decode wherever no two products of a column tie.
 *
 * mr_ctc2d_marginal: out[n, c, w] = reduce over h of classify[n, c, h, w] * mask[n, 0, h, w].
 *   classify at classify + n*cn + c*cc + h*ch + w*cw, mask at mask + n*mn + h*mh + w*mw (element strides, as mr_ctc2d_greedy_decode
 *   takes them); both MR_DTYPE_F32 or both MR_DTYPE_BF16, converted to f32 on load.  out: f32 at out + n*on + c*oc + w*ow.
 *   Arithmetic, the same bits whatever the strides, the tile or the launch: every product is rounded to f32 on its own; reduce == 0
 *   adds them in ascending h, one f32 addition each, starting from the product of h = 0 (nothing fused, nothing reassociated);
 *   reduce == 1 takes fmaxf in the same order.  H == 0 gives 0.  With log_out == 1 the result is replaced by the f32 nearest to its
 *   log (taken in f64 and rounded once; 0 gives -inf): the lp the CTC readers define for log_probs == 0, so passing the logs with
 *   log_probs == 1 gives them the bits they would compute themselves.
 *   One launch, capturable.  classify is read once, the mask once per tile of 32 classes x 32 columns.  Two thread mappings, by the
 *   strides: cc == 1 (an NHWC buffer viewed as NCHW, the project's own head) reads along the classes, everything else along the
 *   columns (a contiguous NCHW tensor: cw == 1); other strides are correct, not fast.  The stores run along w either way.
 *   N, C, H, W >= 0; N, C or W == 0 returns MR_OK without a launch, and pointers may be null only where their tensor has no element.
 *   MR_ERR_ARG, nothing written: a negative size, reduce or log_out outside {0, 1}, sizes times strides beyond a 64-bit offset, more
 *   than INT_MAX tiles, a null pointer; MR_ERR_DTYPE: another dtype code.
 *
 * mr_ctc2d_char_rows: WHERE an alignment lies vertically.  Given a 1-D alignment the heights of its columns are independent, so the
 *   most probable height of a column is an arg-max of its own.  targets i32 [N, S] / target_len i32 [N] and pos i32 [N, W], begin /
 *   end i32 [N, S] as mr_ctc_align took and wrote them for the sum-marginal of the same classify and mask.
 *   rows i32 [N, W]: for column w with position s = pos[n, w] in 0..2K (K = target_len[n] clamped to [0, S]) and class c = blank
 *   for even s, targets[n, s / 2] for odd s: the h with the greatest f32-rounded product classify[n, c, h, w] * mask[n, 0, h, w], the
 *   lowest h among equal values (the product of h = 0 stands until one is greater).  -1 where pos is outside 0..2K (mr_ctc_align
 *   writes -1 for a row it could not align) or c is no class.
 *   row_lo, row_hi i32 [N, S]: for symbol i < K with 0 <= begin < end <= W the least and the greatest rows[n, w] over w in
 *   [begin, end); -1 for every other slot.  All three are written for every row, nothing to be zeroed.
 *   One wave per row, one launch, no host work that depends on device data: capturable.  Only the class a column's position names
 *   is read: S + 1 classes of a row, whatever C is.
 *   N == 0 returns MR_OK without a launch.  MR_ERR_ARG, nothing written: N < 0, C, H or W < 1, S outside
 *   0..MR_CTC_ALIGN_MAX_SYMBOLS, blank outside [0, C), sizes times strides beyond a 64-bit offset, a null pointer (targets, begin,
 *   end, row_lo, row_hi may be null when S == 0); MR_ERR_DTYPE: another dtype code. */
int mr_ctc2d_marginal(int dtype, const void* classify, long long cn, long long cc, long long ch, long long cw,
                      const void* mask, long long mn, long long mh, long long mw, int N, int C, int H, int W,
                      int reduce, int log_out, float* out, long long on, long long oc, long long ow, hipStream_t stream);
int mr_ctc2d_char_rows(int dtype, const void* classify, long long cn, long long cc, long long ch, long long cw,
                       const void* mask, long long mn, long long mh, long long mw, int N, int C, int H, int W, int blank,
                       const int* targets, int S, const int* target_len, const int* pos, const int* begin, const int* end,
                       int* rows, int* row_lo, int* row_hi, hipStream_t stream);

/* ---- Reading with the attention decoder (csrc/attn_read.hip, csrc/attn_beam.hip): the probability of the decoded string and of
 * every character, where each character lies on the feature grid, and the n best strings by beam search.  The decode loop
 * (mr_decode_greedy_fwd, or the per-step kernels) leaves its words and its hidden states H_all [S+1][N][H] behind; given those,
 * the attention map of step s depends on H_all[s] alone and its output distribution on H_all[s + 1] alone, so both are computed
 * for all S steps in parallel BEHIND the loop ("replay read") and the loop itself is not touched.
 *
 * mr_attn_read.  Operands MR_DTYPE_F32 or MR_DTYPE_BF16 (hproj, eproj, logits; converted to f32 on load), v f32 [H]:
 *     hproj   row (s, n) at hproj + (s * N + n) * ldh, H values: the attention half of the hidden projection of H_all[s], s < S
 *     eproj   [N][T][H] contiguous: the encoder half (with the bias)
 *     logits  row (s, n) at logits + (s * N + n) * ldl, C values: the output layer of H_all[s + 1]
 *     words   int32, words[n * ldp + s]: the word emitted at step s (the greedy kernel's pred, or a beam hypothesis)
 *     the grid height x width = T positions, t = y * width + x;  1 <= T <= MR_ATTN_READ_MAX_T;  blank in [0, C).
 *   For every (s, n):
 *     att[n][s][t] (f32 [N][S][T], nullable) = softmax_t(e_t), e_t = sum_h v[h] * tanh(hproj[s][n][h] + eproj[n][t][h]) -- the map
 *       step s of the loop computes from the previous state; tanh in the exp2 / rcp form of the attention kernels (absolute error
 *       ~2e-7); e_t added per lane in ascending h (h = 8 lane + q + 512 k for bf16, 4 lane + q + 256 k for f32; lane + 64 k when H
 *       is no multiple of the 16-byte vector) and then over the 64 lanes by the xor tree 32, 16, .., 1; the softmax as
 *       exp(e - max) / sum with the sums of a row taken per lane in ascending t = lane + 64 k and then by the same tree.
 *     moments[n][s][0..3] (f32) = cx, cy, sx, sy: the mean and the standard deviation of (x + 0.5, y + 0.5) under att, in grid
 *       cells; the variance as sum_t att * (x + 0.5 - cx)^2, same order of summation.
 *     sym_lp[n][s] (f32) = log_softmax(logits[s][n])[words[n][s]] = (l_w - max) - log(sum_c exp(l_c - max)), the sum per lane in
 *       ascending c = lane + 64 k, then the tree.  A word outside [0, C) (the -1 of a timed-out row) gives -inf.
 *   A second launch, per row n:
 *     length[n] (i32) = the index of the first `blank` in words[n][0..S), or S when there is none;
 *     score[n] (f32) = sym_lp[n][0] + sym_lp[n][1] + .. + sym_lp[n][min(length, S - 1)] added in that order: the log-probability
 *       of the string, its terminating blank included when it has one.
 *   A workgroup owns one image and up to 8 consecutive steps and reads eproj[n] once for all of them.  Two launches on `stream`,
 *   no allocation, no synchronisation, no host work that depends on device data: capturable in a graph.  Every output is written
 *   for every row; nothing has to be zeroed.  N == 0 returns MR_OK without a launch.  MR_ERR_ARG, nothing launched: S, H or C < 1,
 *   T outside 1..MR_ATTN_READ_MAX_T, height * width != T, blank outside [0, C), ldh < H, ldl < C, ldp < S, (2 H + T) * 4 bytes
 *   above 64 KiB, more than INT_MAX workgroups, a null pointer (only att may be null); MR_ERR_DTYPE: another dtype code.
 *
 * mr_attn_beam_step: the selection of ONE decode step s of a beam search; the B hypotheses of image n are the rows n * B + b of
 *   the per-step kernels, 1 <= B <= MR_ATTN_BEAM_MAX.  logits: row n * B + b at logits + (n * B + b) * ldl, C values, the output
 *   layer of the new states hprime [N * B][H].  State, read and then rewritten in place (one workgroup per image): score f32
 *   [N * B], finished i32 [N * B], length i32 [N * B].  At s == 0 the state is NOT read: slot 0 of every image is live with score 0
 *   (h0 = 0, fed `blank`), every other slot is dead.
 *     Candidates.  A live, unfinished hypothesis b offers (b, c) for every class c with the value
 *       score[b] + ((logit[b][c] - m_b) - log sum_c' exp(logit[b][c'] - m_b)),  m_b = max_c logit[b][c],
 *     all f32, the sum per lane in ascending c = lane + 64 k and then by the xor tree 32, .., 1.  A finished hypothesis offers only
 *     (b, blank) with score[b] unchanged.  A dead slot (score -inf), and a value that is -inf or NaN, offers nothing.
 *     Selection.  The B candidates with the greatest value, in descending order; between equal values (-0 = +0) the smaller
 *     b * C + c comes first.  No length normalisation.  Fewer than B candidates leave dead slots at the end.
 *     Outputs for the new slot j: parent[(s * N + n) * B + j] = b and word[(s * N + n) * B + j] = c (i32 [S][N][B]); score = the
 *     candidate's value; finished = 1 when b was finished or c == blank; length = length[b] when b was finished, else s when
 *     c == blank (the string ended BEFORE this step's blank), else s + 1; feed[n * B + j] = c as int64, the `idx` of mr_gru_fwd2 for
 *     the next step; h_next[n * B + j][0..H) = hprime[n * B + b][0..H) (h_next must not be hprime).  A dead slot: parent 0, word
 *     blank, score -inf, finished 0, length 0.
 *   One launch, no host work that depends on device data: the S steps of a search can be enqueued, and captured, as a whole.
 *   N == 0 returns MR_OK without a launch.  MR_ERR_ARG, nothing launched: s outside [0, S), B out of range, C < 1 or above
 *   INT_MAX / 64, ldl < C, blank outside [0, C), H < 1, a null pointer, h_next == hprime; MR_ERR_DTYPE: another dtype code.
 *
 * mr_attn_beam_trace: after step S - 1 the slots of an image are its hypotheses in descending order of score.  For n and
 *   j < nbest <= B, following parent back from slot j: ids[n][j][s] = the word of step s (i32 [N][nbest][S]; blank from the end of
 *   a finished string on), lengths[n][j] = the length (S for a hypothesis that never emitted blank), scores[n][j] its score,
 *   path[n][j][s] (i32 [N][nbest][S + 1]) = the slot -- the row of the per-step kernels -- the hypothesis occupied ENTERING step s
 *   (path[.][0] = 0, path[.][S] = j): with H_steps [S + 1][N * B][H] holding every step's hprime at [s + 1], its hidden state after
 *   step s is H_steps[s + 1][n * B + path[n][j][s]].  count[n] = the live hypotheses among the nbest; a dead one gets all blank,
 *   length 0, score -inf, path 0.  One launch, capturable.  MR_ERR_ARG: S < 1, B or nbest out of range, N * nbest * (S + 1) above
 *   INT_MAX, a null pointer. */
#define MR_ATTN_READ_MAX_T 4096     /* positions of the feature grid */
#define MR_ATTN_BEAM_MAX 64         /* hypotheses per image */
int mr_attn_read(int dtype, const void* hproj, long long ldh, const void* eproj, const float* v, const void* logits,
                 long long ldl, const int* words, long long ldp, int blank, int N, int S, int T, int H, int C, int height,
                 int width, float* att, float* sym_lp, float* moments, int* length, float* score, hipStream_t stream);
int mr_attn_beam_step(int dtype, const void* logits, long long ldl, const void* hprime, void* h_next, int H, float* score,
                      int* finished, int* length, int* parent, int* word, long long* feed, int s, int S, int N, int B, int C,
                      int blank, hipStream_t stream);
int mr_attn_beam_trace(const int* parent, const int* word, const float* score, const int* finished, const int* length, int S,
                       int N, int B, int nbest, int blank, int* ids, int* lengths, float* scores, int* count, int* path,
                       hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MEGREADER_HIP_H */
