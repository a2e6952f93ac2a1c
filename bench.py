#!/usr/bin/env python
"""bench.py -- training images/s of CRNN + 1-D CTC (BASELINE.json configs[1]) on N MI355X GPUs.

    python bench.py --gpus 1 --steps 50 --warmup 10
    python bench.py --gpus 1 --steps 50 --warmup 10 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = zero_grad + forward + CTC loss + backward (+ RCCL gradient all-reduce for N>1) + fused Adam on a
device-resident synthetic batch of 256 crops of 32x128 per GPU (weak scaling: global batch = 256*N).
Prints ONE JSON line on rank 0, the last line of stdout.  A plain run only sets up, warms up and times the steps of
the headline workload.  With --full the line also carries
  roofline      -- the dominant MFMA kernel: algorithmic FLOPs of its launches / their HIP-event durations
  kernels       -- per-kernel HIP-event times of the same eager pass
  cpu_baseline  -- the oracle (reference restatement, oracle/crnn.py) timed on this box's host cores (rank 0, N=1)
  secondaries   -- the other published configurations (default single-GPU CRNN run)
  strong        -- the strong-scaling measurement (N > 1, weak scaling)
--dump-outputs DIR: after the timed steps the model is put back to its seeded starting state and the timed step is replayed
once; what it computed (loss, sampled parameters and gradients) is written as .npy files.
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

MFMA_PEAK_TFLOPS = {"bf16": 2500.0, "f32": 157.3}  # dense peaks, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK_GBS = 8000.0


CONV_CALLS = ["mr_conv2d_fwd", "mr_conv2d_fwd_stats", "mr_conv2d_dgrad", "mr_conv2d_dgrad_add", "mr_conv2d_dgrad_bnb",
              "mr_conv2d_wgrad", "mr_conv2d_wgrad_tab"]
# dense weight-gradient GEMMs: followed only so that the ones the library RECORDS (deferred, grouped launches) are attributed to
# the mr_tn_flush that launches them -- the grouped kernel of the timed graph, not one launch per problem
TN_DENSE_CALLS = ["mr_gemm_tn", "mr_gemm_tn2"]
GROUPED = "igemm_tn_glds_grouped_kernel<bf16>"
# phases of the composite DCNv2 entry points (include/megreader_hip.h: mr_phase_timer): id -> (label, unit of `work` on the
# materialised-gcol path (bf16), unit on the fused path, launches per record)
DCN_PHASES = {0: ("dcn2_fwd_fused_kernel", "flop", "flop", 1), 1: ("igemm_nt_kernel<dcn gcol GEMM>", "flop", "flop", 1),
              2: ("dcn2_coord_gcol_kernel", "byte", "flop", 1), 3: ("dcn_csr", "byte", "byte", 4),
              4: ("dcn2_dx_gcol_kernel", "byte", "flop", 1), 5: ("dcn2_im2col_kernel", "byte", "byte", 1),
              6: ("igemm_tn_kernel<dcn wgrad GEMM>", "flop", "flop", 1)}
DCN_FUSED_LABELS = {2: "dcn2_coord_fused_kernel", 4: "dcn2_dx_fused_kernel", 6: "dcn2_wgrad_fused_kernel"}


def normalize_conv_call(name, args):
    """The dgrad variants with extra epilogue operands (round 4) and the statistics forward, mapped onto the argument layout of
    the plain call they extend, so that FLOPs / labels are computed in one place."""
    if name == "mr_conv2d_dgrad_add":          # (dtype, dy, w, dx, addend, N, ...)
        return "mr_conv2d_dgrad", args[:4] + args[5:]
    if name == "mr_conv2d_dgrad_bnb":          # (dtype, dy, w, dx, addend, bn_x, bn_y, mean, rstd, sums, produced, N, ...)
        return "mr_conv2d_dgrad", args[:4] + args[11:]
    if name == "mr_conv2d_fwd_stats":          # (dtype, x, w, bias, y, sums, N, H, W, Cin, ldx, Cout, R, ...): no relu / ldy
        a = args
        return "mr_conv2d_fwd", a[:5] + (0,) + a[6:12] + (a[11],) + a[12:]
    return name, args


def conv_flops(name, args, true_cin0=3):
    """algorithmic FLOPs (2*MACs, un-padded channels) of one mr_conv2d_* call from its C-ABI arguments."""
    name, args = normalize_conv_call(name, args)
    if name == "mr_conv2d_fwd":
        N, H, W, Cin, _ldx, Cout, _ldy, R, S = args[6:15]
        Ho, Wo = args[21], args[22]
    elif name == "mr_conv2d_dgrad":
        N, H, W, Cin, _ld1, Cout, _ld2, R, S = args[4:13]
        Ho, Wo = args[19], args[20]
    else:  # wgrad: (dtype, dy, x, dw, dbias, N, H, W, Cin, ldx, Cout, lddy, R, S, ...6..., Ho, Wo)
        N, H, W, Cin, _ld1, Cout, _ld2, R, S = args[5:14]
        Ho, Wo = args[20], args[21]
    if Cin == 8 and Cout == 64:
        Cin = true_cin0  # first layer: 3 input channels padded to one 16-byte vector
    return 2.0 * N * Ho * Wo * Cout * R * S * Cin, N * Ho * Wo, Cout, Cin


COMPOSITE_N = " (several launches)"
COMPOSITE = "+tail (2 launches)"   # a C-ABI call that launches the 256x256 head kernel AND a 4-wave tail kernel


def kernel_label(lib, name, args, dtype_name):
    dt = 1 if dtype_name == "bf16" else 0
    bnb = name == "mr_conv2d_dgrad_bnb"       # stays on the 4-wave tiles (the 8-wave kernels have no BatchNorm-backward epilogue)
    name, args = normalize_conv_call(name, args)

    def nt(code):
        if code == 256257:   # head / tail split (gemm_conv.hip:nt_head_rows): the event bracket spans two kernels
            return "igemm_nt_kernel<%s,256,256,conv>%s" % (dtype_name, COMPOSITE)
        return "igemm_nt_kernel<%s,%d,%d,conv>" % (dtype_name, code // 1000, code % 1000)
    if name == "mr_conv2d_fwd":
        N, H, W, Cin, _ldx, Cout, _ldy, R, S = args[6:15]
        return nt(lib.mr_nt_kernel_code(dt, N * args[21] * args[22], Cout, R * S * Cin, Cin))
    if name == "mr_conv2d_dgrad":
        N, H, W, Cin, _ld1, Cout, _ld2, R, S = args[4:13]
        if bnb:
            code = lib.mr_nt_tile_code(N * H * W, Cin)
            return "igemm_nt_kernel<%s,%d,%d,conv+bn_bwd_sums>" % (dtype_name, code // 1000, code % 1000)
        return nt(lib.mr_nt_kernel_code(dt, N * H * W, Cin, R * S * Cout, Cout))
    # wgrad: (dtype, dy, x, dw, dbias, N, H, W, Cin, ldx, Cout, lddy, R, S, sh, sw, ph, pw, dh, dw, Ho, Wo[, tab, build])
    if name == "mr_conv2d_wgrad_tab" and dt == 1 and args[22] and lib.mr_tn_taps_would_run(*[int(v) for v in args[5:22]]):
        return "igemm_tn_taps_kernel<bf16,3x3>"   # all-taps kernel (csrc/tn_taps.hip)
    return "igemm_tn_kernel<%s,conv>" % dtype_name


def write_shape_table(path, lib, results, dtype_name, steps):
    """Per-(entry point, geometry) statistics of the event-bracketed convolution launches of `steps` eager steps (--shape-table):
    the table the tile / split heuristics are read against.  Columns: launches per step, average microseconds, algorithmic
    TFLOP/s, entry, kernel label, M x N x K of the implicit GEMM, geometry."""
    rows = {}
    for name, cargs, t_ms in results:
        n0, a0 = normalize_conv_call(name, cargs)
        if n0 == "mr_conv2d_fwd":
            N, H, W, Cin, _l, Cout, _l2, R, S, sh, sw = a0[6:17]
            Ho, Wo = a0[21], a0[22]
            M, Nn, K = N * Ho * Wo, Cout, R * S * Cin
        elif n0 == "mr_conv2d_dgrad":
            N, H, W, Cin, _l, Cout, _l2, R, S, sh, sw = a0[4:15]
            Ho, Wo = a0[19], a0[20]
            M, Nn, K = N * H * W, Cin, R * S * Cout
        else:
            N, H, W, Cin, _l, Cout, _l2, R, S, sh, sw = a0[5:16]
            Ho, Wo = a0[20], a0[21]
            M, Nn, K = Cout, R * S * Cin, N * Ho * Wo
        key = (name, kernel_label(lib, name, cargs, dtype_name), M, Nn, K, "%dx%d s%d %dx%d->%dx%d" % (R, S, sh, H, W, Ho, Wo))
        r = rows.setdefault(key, [0, 0.0, conv_flops(name, cargs)[0]])
        r[0] += 1
        r[1] += t_ms
    with open(path, "w") as f:
        f.write("per_step  avg_us  tflops  entry  kernel  M N K  geometry\n")
        for key, (n, t_ms, fl) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
            f.write("%5.1f %8.2f %7.1f  %-22s %-44s %7d %6d %7d  %s\n" %
                    (n / steps, 1e3 * t_ms / n, fl / (t_ms / n * 1e-3) / 1e12, key[0], key[1], key[2], key[3], key[4], key[5]))


def kernel_source_hash():
    """sha256 over megreader_amd/csrc/*.hip, *.h (same function as tools/pmc_to_json.py, which stamps it into the PMC file)."""
    import hashlib
    here = os.path.join(REPO, "megreader_amd", "csrc")
    h = hashlib.sha256()
    for name in sorted(os.listdir(here)):
        if name.endswith((".hip", ".h")):
            h.update(name.encode())
            h.update(open(os.path.join(here, name), "rb").read())
    return h.hexdigest()[:16]


def pmc_traffic(label, workload="crnn"):
    """HBM-side bytes per launch of `label` from the committed PMC passes (profiles/rNN_pmc_traffic_<workload>.json, produced
    by tools/profile_r04.sh + tools/pmc_to_json.py: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same
    command, FETCH_SIZE doubled for gfx950).  PMC counters cannot be read inside this process, so each file is stamped with a
    hash of the kernel sources it was measured on: the newest file whose stamp equals the current sources is used; if none
    does (kernels edited since) traffic = null instead of a number that no longer describes the code."""
    import glob
    prof = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
    paths = sorted(glob.glob(os.path.join(prof, "r[0-9][0-9]_pmc_traffic_%s.json" % workload)), reverse=True)
    current = kernel_source_hash()
    stale = None
    for path in paths:
        try:
            data = json.load(open(path))
        except (OSError, ValueError):
            continue
        name = os.path.basename(path)
        if data.get("_kernel_source_hash") != current:
            stale = stale or "profiles/%s is stale (measured on kernel sources %s, current %s)" % \
                (name, data.get("_kernel_source_hash"), current)
            continue
        if label not in data:
            return None, None
        return data[label]["bytes_per_launch"], "profiles/%s (rocprofv3 --pmc, %d launches)" % \
            (name, data[label]["launches"])
    return None, stale


def _host_threads():
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    return max(1, min(avail, 32)), avail  # more threads than this only add contention at these tensor sizes


def cpu_baseline(workload="crnn", budget_s=20.0, crop=None):
    """The oracle restatement of the reference model (oracle/: torch CPU kernels, fp32 weights, the reference's own fp64 /
    numpy CTC -- what the reference executes on a CPU) timed on this box's host cores: a BOUNDED sample of the same workload
    (one warm-up step, then whole training steps until about half the budget is used; at least one).  CRNN runs at the
    benchmarked batch 256; the three bigger models at a smaller batch, stated in `sample`.  kind = "port"."""
    threads, avail = _host_threads()
    torch.set_num_threads(threads)
    torch.manual_seed(0)
    if workload == "crnn":
        from oracle.crnn import CRNNOracle, synthetic_batch
        model, n = CRNNOracle().train(), 256
        batch = synthetic_batch(n, 32, 128, seed=0)
        what = "batch 256 (32x128 crops, the benchmarked batch)"
    elif workload == "res50ppm":
        from oracle.res50ppm import Res50PPM2DCTCOracle, synthetic_batch_2d
        ch, cw = crop or (32, 128)
        model, n = Res50PPM2DCTCOracle().train(), (64 if ch * cw <= 32 * 128 else 16)
        batch = synthetic_batch_2d(n, ch, cw, seed=0, max_len=3)
        what = "batch %d of the benchmarked 256 (%dx%d crops)" % (n, ch, cw)
    elif workload == "fpn_attention":
        from oracle.crnn import synthetic_batch
        from oracle.fpn_attention import FPNAttentionOracle
        model, n = FPNAttentionOracle().train(), 32
        batch = synthetic_batch(n, 64, 256, seed=0)
        what = "batch 32 (64x256 crops, the benchmarked per-GPU batch), gt_as_output fixed"
    else:
        from megreader_amd.synthetic import detection_batch
        from oracle.res50ppm import _Res50Dilated
        from oracle.seg_detector import SegDetectorOracle, l1_balance_ce_loss

        class DB(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.backbone = _Res50Dilated(dilate=False, dcn=True)
                self.decoder = SegDetectorOracle(in_channels=[256, 512, 1024, 2048], adaptive=True, k=50)

            def forward(self, image):
                return self.decoder(self.backbone(image))
        model, n = DB().train(), 2
        batch = detection_batch(n, 640, seed=0)
        what = "batch 2 (640x640 images, the benchmarked per-GPU batch); DCNv2 = the float32 torch restatement (oracle/dcn.py)"
    if workload == "db":
        opt = torch.optim.SGD(model.parameters(), lr=0.007, momentum=0.9, weight_decay=1e-4)

        def step():
            opt.zero_grad()
            loss = l1_balance_ce_loss(model(batch['image']), batch)
            loss.backward()
            opt.step()
    else:
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        lab, ln = batch['label'], batch['length'].long()

        def step():
            opt.zero_grad()
            loss, _ = model(batch['image'], targets=lab, lengths=ln, train=True)
            loss.mean().backward()
            opt.step()
    t0 = time.perf_counter()
    step()  # warm-up
    warm = time.perf_counter() - t0
    max_steps = 20 if warm < 0.25 * budget_s else 1
    t0 = time.perf_counter()
    steps = 0
    while steps < max_steps and (steps < 1 or time.perf_counter() - t0 < 0.5 * budget_s):
        step()
        steps += 1
    dt = time.perf_counter() - t0
    return {"value": round(n * steps / dt, 2), "unit": "images/s", "cores": threads, "kind": "port",
            "sample": "%d CPU training step(s) at %s with the oracle restatement of the reference model, torch %s CPU kernels, "
                      "%d threads (%d cores visible), %.1f s after one warm-up step of %.1f s" %
                      (steps, what, torch.__version__, threads, avail, dt, warm)}


DUMP_SAMPLE = 1 << 22     # elements per sampled array: 2 x 16 MB of float32 at most


def seeded_state(model, opt):
    """--dump-outputs: the seeded starting point of the run (taken before the first step): the flat fp32 parameters of every
    optimizer group and the model's buffers.  The moments and the step counter are zero at that point."""
    return ([f['p'].clone() if f is not None else None for f in opt._flat], [b.detach().clone() for b in model.buffers()])


def restore_seeded_state(model, opt, state):
    """Put the model and its fused optimizer back to `state` IN PLACE (a captured step keeps reading the same buffers):
    parameters and buffers copied back, moments zeroed, the compute-dtype operand images regenerated from the restored
    parameters, and the device step counter (hyper[5], completed steps) back to zero -- the update of the next step is then
    the first one again, bias correction included."""
    from megreader_amd.nn import prep
    flat_p, bufs = state
    for f, p0 in zip(opt._flat, flat_p):
        if f is None:
            continue
        f['p'].copy_(p0)
        f['s1'].zero_()
        f['s2'].zero_()
        prep.refresh(f['params'], f, tick=f['hyper'])      # regenerates the images; advances the counter ...
        f['hyper'][5:6].zero_()                            # ... which is reset behind it
    for b, b0 in zip(model.buffers(), bufs):
        b.copy_(b0)


def dump_outputs(out_dir, loss, model):
    """--dump-outputs: what one step of the timed path handed its caller, as .npy files in `out_dir`: the step's loss
    (float64) and the model after the step -- its parameters and their gradients, each flattened in `model.parameters()`
    order and, when longer than DUMP_SAMPLE, reduced to a fixed sample (sorted indices drawn with seed 0).
    The step is the timed path (the captured graph, or the eager step with --no-graph) replayed once after the timed steps
    from the seeded starting state (restore_seeded_state): its inputs are then the same in every run.  The inputs of the
    last TIMED step are not: they are the product of all the updates before it, and the step is not bit-repeatable (float
    atomics in split reductions and BatchNorm statistics), a difference of rounding that Adam's normalised update turns into
    different weights within tens of steps."""
    import numpy as np
    params = [p for p in model.parameters()]
    flat_p = torch.cat([p.detach().reshape(-1).float() for p in params])
    flat_g = torch.cat([p.grad.detach().reshape(-1).float() if p.grad is not None
                        else torch.zeros(p.numel(), device=p.device) for p in params])
    n = flat_p.numel()
    if n > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(0).choice(n, DUMP_SAMPLE, replace=False))
        sel = torch.from_numpy(idx).to(flat_p.device)
        flat_p, flat_g = flat_p[sel], flat_g[sel]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), np.array([loss], dtype=np.float64))
    np.save(os.path.join(out_dir, "params.npy"), flat_p.cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "grads.npy"), flat_g.cpu().numpy().astype(np.float32))


def quiet_native_stdout():
    """Ranks other than 0 print nothing of their own, but RCCL writes a version banner through C stdio into THEIR stdout, which
    torch.distributed.run forwards to the launcher's: send file descriptor 1 of those ranks to stderr for the whole run."""
    sys.stdout.flush()
    os.dup2(2, 1)


def emit_last_line(line):
    """Print the result as the LAST line of stdout.  Native libraries (RCCL's version banner) hold text in the C stdio buffer
    that libc flushes at exit, i.e. after everything Python printed: flush it first, print the JSON line, then point file
    descriptor 1 at /dev/null so that nothing flushed later can follow it."""
    import ctypes
    try:
        ctypes.CDLL(None).fflush(None)
    except Exception:  # noqa: BLE001 - no libc handle: the dup2 below still keeps later output away
        pass
    sys.stdout.flush()
    if line is not None:
        sys.stdout.write(line + "\n")
        sys.stdout.flush()
    devnull = os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 1)
    os.close(devnull)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)     # >= 50 timed steps after >= 10 warm-up
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the secondary measurements (configs[2..4]) of the default single-GPU run")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak (default): --batch crops PER GPU, global batch = batch x N.  strong: the reference's rule "
                         "(data/data_loader.py:40-48 `batch_size // world_size`): the workload's GLOBAL batch (256 crops; 16 "
                         "images for db) is sharded over the N ranks, --batch is then the global batch")
    ap.add_argument("--no-kernel-timer", action="store_true")
    ap.add_argument("--crop", default="", metavar="HxW",
                    help="res50ppm only: crop size (default 32x128 = BASELINE.json configs[2] as benchmarked since round 1; 64x256 = "
                         "the YAML-native size of experiments/recognition/community-base.yaml:33-35, BASELINE.md C3)")
    ap.add_argument("--no-strong", action="store_true",
                    help="N > 1, weak scaling: do not append the strong-scaling measurement (the workload's GLOBAL batch sharded "
                         "over the ranks, data/data_loader.py:40-48) as a `strong` block to the JSON line")
    ap.add_argument("--no-graph", action="store_true", help="time eager launches instead of a hipGraph replay")
    ap.add_argument("--shape-table", default="", help="write per-geometry statistics of the convolution launches to this file")
    ap.add_argument("--force-ddp", action="store_true",
                    help="take the multi-GPU code path even with WORLD_SIZE=1 (single-GPU test of that path)")
    ap.add_argument("--ddp-mode", default="auto", choices=["auto", "capture", "graph2"],
                    help="N > 1 with hipGraph replay: 'capture' = the apex-style shim's bucketed RCCL all-reduces are "
                         "captured INSIDE the step graph on a side stream (overlapped with backward, zero host cost); "
                         "'graph2' = two graphs with one eager all-reduce between them (not overlapped); 'auto' = "
                         "capture, falling back to graph2 if the capture fails")
    ap.add_argument("--tn-model", type=int, default=-1, help="A/B: mr_set_tn_model (wgrad split model), -1 = default")
    ap.add_argument("--set", action="append", default=[], metavar="NAME=INT",
                    help="A/B: call the host-only tuning setter mr_set_NAME(INT) before the run (e.g. --set nt_deep=0); "
                         "recorded in config.tuning")
    ap.add_argument("--teacher-forcing", default="fixed", choices=["fixed", "random"],
                    help="fpn_attention: fixed = gt_as_output=True (default, deterministic); random = the YAML default (a coin per "
                         "decode step, decoders/attention_decoder.py:50-54)")
    ap.add_argument("--workload", default="crnn", choices=["crnn", "res50ppm", "fpn_attention", "db"],
                    help="crnn = BASELINE.json configs[1] (the metric's workload, default); res50ppm = configs[2]: "
                         "ResNet50-dilated-PPM + 2D-CTC on 32x128 crops (secondary line, same JSON shape); "
                         "fpn_attention = configs[3]: ResNet50-FPN + attention decoder on 64x256 crops, batch 32 per "
                         "GPU (256 global on 8 GPUs), gt_as_output fixed for determinism; db = configs[4]: the DB detector "
                         "(deformable ResNet-50 with 13 DCNv2 layers + SegDetector + L1BalanceCELoss, SGD) on 640x640 "
                         "images, batch 2 per GPU (16 global on 8 GPUs)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: the eager kernel-timer pass (roofline, kernels), "
                         "the CPU baselines, the secondary configurations and, for N > 1, the strong-scaling line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, replay the timed step once from the seeded starting state and write what "
                         "it computed as DIR/<name>.npy: loss (float64), and a fixed, seeded sample of the updated parameters "
                         "and of their gradients (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.shape_table and not args.full:
        ap.error("--shape-table needs --full (it is written from the eager kernel-timer pass)")
    kernel_timer = args.full and not args.no_kernel_timer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an AMD GPU (there is no CPU product path)")
    if args.tn_model >= 0:
        from megreader_amd import _lib as _l
        _l.load().mr_set_tn_model(args.tn_model)
    for kv in args.set:
        from megreader_amd import _lib as _l
        name, val = kv.split("=")
        _lib_ = _l.load()
        if name in _l.TUNING_FIELDS and not hasattr(_lib_, "mr_set_" + name):
            _l.set_tuning(**{name: int(val)})       # a plain mr_tuning field
        else:
            getattr(_lib_, "mr_set_" + name)(int(val))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    distributed = world > 1 or args.force_ddp
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rank != 0:
            quiet_native_stdout()
        dist.init_process_group(backend="nccl", init_method="env://")
    if args.gpus != world:
        print("warning: --gpus %d but WORLD_SIZE %d (using WORLD_SIZE)" % (args.gpus, world), file=sys.stderr)

    def measure(workload, steps, warmup, with_cpu, scaling=None, crop=None, coins=None, dump_dir=""):
        """One workload: build, warm up, time `steps` steps; returns the result dict on rank 0 (None elsewhere).  With a
        `dump_dir`, rank 0 writes what the last timed step computed there (dump_outputs)."""
        scaling = scaling or args.scaling
        random_coins = (coins or args.teacher_forcing) == "random"
        if crop is None and args.crop and workload == "res50ppm":
            crop = tuple(int(v) for v in args.crop.lower().split("x"))
        import megreader_amd as mr
        from megreader_amd import _lib
        from megreader_amd.backbones import crnn_backbone
        from megreader_amd.decoders import CRNNDecoder
        from megreader_amd.optim import FusedAdam
        from megreader_amd.runtime import scalar_mean
        from megreader_amd.synthetic import recognition_batch as synthetic_batch  # BASELINE.md §3 value distributions

        lib = _lib.load()
        dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
        mr.set_compute_dtype(dtype)
        from megreader_amd.nn import functional as _Fn
        _Fn.LSTM_STATUS = lstm_status = []      # status words of the persistent-recurrence workspaces (checked after the timed region)

        class BasicModel(torch.nn.Module):  # reference structure/model.py:16-24
            def __init__(self):
                super().__init__()
                self.backbone = crnn_backbone()
                self.decoder = CRNNDecoder(in_channels=512, inner_channels=256)

            def forward(self, data, *a, **k):
                return self.decoder(self.backbone(data), *a, **k)

        if workload == "res50ppm":
            from megreader_amd.backbones import resnet50dilated_ppm
            from megreader_amd.decoders import CTCDecoder2D
            from megreader_amd.synthetic import recognition_batch_2d as synthetic_batch_2d

            class BasicModel(torch.nn.Module):  # noqa: F811  res50-ppm-2d-ctc.yaml: resnet50dilated_ppm + CTCDecoder2D
                def __init__(self):
                    super().__init__()
                    self.backbone = resnet50dilated_ppm()
                    self.decoder = CTCDecoder2D(in_channels=256)

                def forward(self, data, *a, **k):
                    return self.decoder(self.backbone(data), *a, **k)

        if workload == "fpn_attention":
            from megreader_amd.backbones import Resnet50FPN
            from megreader_amd.decoders import AttentionDecoder

            class BasicModel(torch.nn.Module):  # noqa: F811  fpn50-attention-decoder.yaml: Resnet50FPN + AttentionDecoder
                def __init__(self):
                    super().__init__()
                    self.backbone = Resnet50FPN(resnet_pretrained=False)     # no network on the box
                    # coins: 'fixed' = teacher forcing on every step (gt_as_output=True, the benchmarked configuration since
                    # round 2); 'random' = the YAML default of fpn50-attention-decoder.yaml (gt_as_output=None: a device-resident
                    # coin per decode step, decoders/attention_decoder.py:50-54), which keeps the output layer on the recurrence
                    self.decoder = AttentionDecoder(in_channels=256, gt_as_output=True if random_coins is False else None)

                def forward(self, data, *a, **k):
                    return self.decoder(self.backbone(data), *a, **k)

        is_db = workload == "db"
        if is_db:
            from megreader_amd.backbones import deformable_resnet50
            from megreader_amd.decoders import L1BalanceCELoss, SegDetector
            from megreader_amd.optim import FusedSGD
            from megreader_amd.synthetic import detection_batch

            class BasicModel(torch.nn.Module):  # noqa: F811  seg_detector_db.yaml:47-62 (SegDetectorModel + its loss)
                def __init__(self):
                    super().__init__()
                    self.backbone = deformable_resnet50(pretrained=False)
                    self.decoder = SegDetector(in_channels=[256, 512, 1024, 2048], adaptive=True, k=50)
                    self.criterion = L1BalanceCELoss()

                def forward(self, batch):
                    pred = self.decoder(self.backbone(batch['image']))
                    return self.criterion(pred, batch)

        torch.manual_seed(0)
        model = BasicModel().to(dev).train()
        if is_db:   # seg_detector_db.yaml:85-94: SGD momentum 0.9, weight decay 1e-4, lr 0.007
            opt = FusedSGD(model.parameters(), lr=0.007, momentum=0.9, weight_decay=1e-4)
        else:
            opt = FusedAdam(model.parameters(), lr=1e-3)  # experiments/recognition/crnn.yaml:82-89 (both YAMLs use Adam)
        opt.zero_grad()
        net = model
        use_graph = not args.no_graph   # the DB loss keeps its hard-negative count on the device (seg_detector_loss.py)
        if distributed and not use_graph:
            # eager data parallel: the apex-style shim (bucketed all-reduce overlapped with backward)
            from megreader_amd.apex.parallel import DistributedDataParallel
            net = DistributedDataParallel(model)
            net.fold_average_into(opt)     # 1 / world applied inside the fused update kernel (no flat.mul_ pass)
        elif distributed:
            # graphed data parallel; rank 0's weights define the model.  The shim is constructed here (it broadcasts) and
            # used by the 'capture' mode; 'graph2' works on the bare model with an eager flat all-reduce between two graphs
            from megreader_amd.apex.parallel import DistributedDataParallel
            ddp_shim = DistributedDataParallel(model)
            ddp_shim.fold_average_into(opt)
        seeded = seeded_state(model, opt) if dump_dir else None    # before the first step
        bsz = args.batch
        if scaling == "strong":
            # the reference shards ONE global batch: per-rank batch = global // world (data/data_loader.py:40-48)
            glob = args.batch if args.batch != 256 else (16 if is_db else 256)
            if glob % world:
                raise SystemExit("--scaling strong: global batch %d is not divisible by %d ranks" % (glob, world))
            bsz = glob // world
        if is_db:
            if scaling != "strong":
                bsz = args.batch if args.batch != 256 else 2           # configs[4]: 16 global = 2 per GPU on 8 GPUs
            dbatch = {k: v.to(dev) for k, v in detection_batch(bsz, 640, seed=rank).items()}
            batch = {'image': dbatch['image'], 'label': torch.zeros(1), 'length': torch.zeros(1)}
        elif workload == "res50ppm":
            ch, cw = crop or (32, 128)
            batch = synthetic_batch_2d(bsz, ch, cw, seed=rank, max_len=3)
        elif workload == "fpn_attention":
            if scaling != "strong":
                bsz = args.batch if args.batch != 256 else 32      # configs[3]: 256 global = 32 per GPU on 8 GPUs
            batch = synthetic_batch(bsz, 64, 256, seed=rank)
        else:
            batch = synthetic_batch(bsz, 32, 128, seed=rank)
        img = batch['image'].to(dev)
        lab = batch['label'].to(dev)
        ln = batch['length'].to(dev).long()

        def step():
            opt.zero_grad()
            if is_db:
                loss, _ = net(dbatch)
            else:
                loss, _ = net(img, targets=lab, lengths=ln, train=True)
            loss = scalar_mean(loss)     # trainer.py:124 `l.mean()`; a 0-dim loss is its own mean (no launch)
            loss.backward()
            opt.step()
            return loss

        def barrier():
            if distributed:
                dist.barrier()
            torch.cuda.synchronize()

        for _ in range(warmup if not (distributed and use_graph) else 0):
            step()
        graphed = None
        if use_graph:
            # the whole step (zero_grad, forward, CTC, backward, fused Adam) as ONE captured hipGraph; the timed region
            # replays it.  Same kernels, same work -- only the ~150 host-side launches per step are gone.
            from megreader_amd.runtime import GraphedTrainStep, data_parallel_grad_sync

            def loss_fn(i, l, n):
                if is_db:
                    loss, _ = net(dbatch)
                    return scalar_mean(loss)
                loss, _ = net(i, targets=l, lengths=n, train=True)
                return scalar_mean(loss)

            ddp_launch = None
            if distributed and args.ddp_mode in ("auto", "capture"):
                # ONE graph: forward, backward with the shim's per-bucket all-reduces on its side stream (captured as a
                # parallel branch: they overlap the rest of backward), finalisation, fused Adam
                try:
                    net = ddp_shim
                    graphed = GraphedTrainStep(loss_fn, opt, [img, lab, ln], warmup=max(2, warmup), grad_sync=None)
                    ddp_launch = "hipGraph replay with in-graph bucketed RCCL all-reduce (overlapped with backward)"
                except Exception as e:  # noqa: BLE001 - any capture failure falls back to the two-graph path
                    if args.ddp_mode == "capture":
                        raise
                    print("in-graph collective capture failed (%s: %s); falling back to --ddp-mode graph2" %
                          (type(e).__name__, e), file=sys.stderr)
                    torch.cuda.synchronize()
                    net = model
                    graphed = None
            if graphed is None:
                net = model
                if distributed:
                    ddp_shim.suspended = True      # its parameter hooks stay registered: the eager all-reduce below replaces them
                    ddp_shim.unfold_average()
                sync = data_parallel_grad_sync(opt, fold=True) if distributed else None
                graphed = GraphedTrainStep(loss_fn, opt, [img, lab, ln], warmup=max(2, warmup if distributed else 2),
                                           grad_sync=sync)
                if distributed:
                    ddp_launch = "2 hipGraphs + eager in-place RCCL all-reduce of the flat gradients"
            run = graphed
        else:
            run = step
        timer = None
        if kernel_timer and not use_graph:
            timer = _lib.KernelTimer(CONV_CALLS)
            _lib.TIMER = timer
        barrier()
        t0 = time.perf_counter()
        last = None
        for _ in range(steps):
            last = run()
        host_enqueue = time.perf_counter() - t0   # host time to enqueue all steps (GPU still running)
        barrier()
        elapsed = time.perf_counter() - t0
        _lib.TIMER = None
        final_loss = float(last.detach())
        # the persistent BiLSTM / one-pass BatchNorm kernels POISON their outputs with NaN when a bounded spin times out
        # (lstm_persist.hip:30, norm_pool.hip): a non-finite loss or a raised status word on ANY rank voids the measurement
        bad = 0 if math.isfinite(final_loss) else 1
        lstm_words = [int(t.view(torch.int32).item()) for t in lstm_status[-8:]]
        _Fn.LSTM_STATUS = None
        if any(lstm_words):
            bad |= 2
        if distributed:
            tb = torch.tensor([bad], device=dev, dtype=torch.int32)
            dist.all_reduce(tb, op=dist.ReduceOp.MAX)
            bad = int(tb)
        if bad:
            raise RuntimeError("bench.py: invalid step on some rank -- %s%s (rank %d: final loss %r, LSTM status words %r)" %
                               ("non-finite loss " if bad & 1 else "", "persistent-kernel (LSTM / decode) timeout" if bad & 2 else "", rank,
                                final_loss, lstm_words))
        if dump_dir:
            # one more step of the timed path, untimed, from the seeded starting state (every rank: the step may hold
            # collectives); written before the kernel-timer pass below runs further steps
            restore_seeded_state(model, opt, seeded)
            dump_loss = float(run().detach())
            barrier()
            if not math.isfinite(dump_loss):
                raise RuntimeError("bench.py: non-finite loss in the step replayed for --dump-outputs (%r)" % dump_loss)
            if rank == 0:
                dump_outputs(dump_dir, dump_loss, model)
        if use_graph and kernel_timer:
            # HIP events cannot bracket kernels inside a graph replay: measure the dominant kernel's launch durations
            # on the same stream with the same tensors in an eager pass right after the timed region
            # (deferred weight-gradient problems are launched grouped, from mr_tn_flush: an event bracket around the recording
            # call would time nothing, so this pass launches every problem on its own -- the grouped launches of the timed
            # region are in the rocprofv3 summaries under profiles/)
            # (round 6: deferred weight-gradient problems stay deferred -- the bracket goes around the mr_tn_flush that launches
            # them grouped, as in the timed graph; the DCNv2 entry points time their own launches, mr_phase_timer)
            timer = _lib.KernelTimer(CONV_CALLS + TN_DENSE_CALLS, track_deferred=True)
            _lib.TIMER = timer
            timer_steps = min(steps, 10)
            lib.mr_phase_timer(1)
            try:
                for _ in range(timer_steps):
                    step()
                torch.cuda.synchronize()
            finally:
                _lib.TIMER = None
                lib.mr_phase_timer(0)
        else:
            timer_steps = steps
        if distributed:
            t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t)

        if rank == 0:
            ms = 1e3 * elapsed / steps
            images = bsz * world * steps
            # ---- roofline of the dominant MFMA kernel from the live HIP-event records
            roofline = None
            kernels = {}
            if timer is not None:
                agg = {}
                algo_bytes = {}
                es = 2 if args.dtype == "bf16" else 4

                def problem(name, cargs):
                    """(flops, algorithmic bytes) of one recorded C-ABI call"""
                    if name in TN_DENSE_CALLS:      # (dtype, A, lda, B, ldb, C, ldc, P, NA, NB, ...): C[NA, NB] += A^T B over P rows
                        P_, NA_, NB_ = cargs[7], cargs[8], cargs[9]
                        return 2.0 * P_ * NA_ * NB_, es * P_ * (NA_ + NB_) + 4.0 * NA_ * NB_
                    fl, pix, cout, cin = conv_flops(name, cargs)
                    # both activation tensors once + the weights once
                    return fl, es * (pix * cout + pix * cin) + es * fl / (2.0 * pix)

                conv_records = []
                for name, cargs, t_ms in timer.results():
                    if name == "mr_tn_flush":       # cargs = the recorded problems this flush launched as ONE grouped kernel
                        label, fl, ab = GROUPED, 0.0, 0.0
                        for pn, pa in cargs:
                            f1, b1 = problem(pn, pa)
                            fl += f1
                            ab += b1
                    elif name in TN_DENSE_CALLS:
                        continue                    # an immediate dense wgrad launch (LSTM / Linear layers): not a conv kernel
                    else:
                        label = kernel_label(lib, name, cargs, args.dtype)
                        fl, ab = problem(name, cargs)
                        conv_records.append((name, cargs, t_ms))
                    algo_bytes[label] = algo_bytes.get(label, 0.0) + ab
                    a = agg.setdefault(label, [0.0, 0.0, 0])
                    a[0] += fl
                    a[1] += t_ms
                    a[2] += 1
                # DCNv2 phases (db): per-kernel HIP-event times recorded inside mr_dcn2_fwd / mr_dcn2_bwd2
                hbm_kernels = {}
                gcol_path = args.dtype == "bf16" and _lib.get_tuning().get("dcn_gcol", 0) == 1
                for pid, (plabel, unit_gcol, unit_fused, nlaunch) in DCN_PHASES.items():
                    ms_c, work_c = ctypes.c_double(0.0), ctypes.c_double(0.0)
                    n = lib.mr_phase_read(pid, ctypes.byref(ms_c), ctypes.byref(work_c))
                    if n <= 0:
                        continue
                    unit = unit_gcol if gcol_path else unit_fused
                    if not gcol_path and pid in DCN_FUSED_LABELS:
                        plabel = DCN_FUSED_LABELS[pid]
                    if nlaunch > 1:
                        plabel += COMPOSITE_N
                    if unit == "flop":
                        agg[plabel] = [work_c.value, ms_c.value, n]
                    else:
                        hbm_kernels[plabel] = [work_c.value, ms_c.value, n]
                if args.shape_table:
                    write_shape_table(args.shape_table, lib, conv_records, args.dtype, timer_steps)
                for label, (fl, t_ms, n) in agg.items():
                    kernels[label] = {"launches_per_step": n / timer_steps, "avg_us": round(1e3 * t_ms / n, 2),
                                      "tflops": round(fl / (t_ms * 1e-3) / 1e12, 1),
                                      "ms_per_step": round(t_ms / timer_steps, 4)}
                for label, (by, t_ms, n) in hbm_kernels.items():
                    kernels[label] = {"launches_per_step": n / timer_steps, "avg_us": round(1e3 * t_ms / n, 2),
                                      "gbytes_per_s": round(by / (t_ms * 1e-3) / 1e9, 1), "ms_per_step": round(t_ms / timer_steps, 4)}
                single = {k: v for k, v in agg.items() if not k.endswith(COMPOSITE) and not k.endswith(COMPOSITE_N)}
                single_hbm = {k: v for k, v in hbm_kernels.items() if not k.endswith(COMPOSITE_N)}
                dom_hbm = max(single_hbm, key=lambda k: single_hbm[k][1]) if single_hbm else None
                dom_mfma = max(single, key=lambda k: single[k][1]) if single else None
                if dom_hbm is not None and (dom_mfma is None or single_hbm[dom_hbm][1] > single[dom_mfma][1]):
                    # the workload's dominant kernel is bandwidth-bound (DB: the CSR gather of the DCNv2 input gradient)
                    by, t_ms, n = single_hbm[dom_hbm]
                    ach = by / (t_ms * 1e-3) / 1e9
                    traffic, traffic_src = pmc_traffic(dom_hbm, workload)
                    roofline = {"kernel": dom_hbm, "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS,
                                "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic,
                                "traffic_unit": "HBM-side bytes per launch", "traffic_source": traffic_src,
                                "algorithmic_bytes_per_launch": round(by / n), "avg_launch_us": round(1e3 * t_ms / n, 2),
                                "launches": n,
                                "measured": "HIP events around the launch inside the C entry point (mr_phase_timer), eager pass "
                                            "after the graph-replayed timed region"}
                elif agg:
                    # the roofline block is ONE kernel (its rocprofv3 average must agree with the event average):
                    # event brackets that span two launches stay in `kernels` but cannot be the dominant kernel
                    single = single or agg
                    dom = max(single, key=lambda k: single[k][1])
                    fl, t_ms, n = agg[dom]
                    ach = fl / (t_ms * 1e-3) / 1e12
                    peak = MFMA_PEAK_TFLOPS[args.dtype]
                    traffic, traffic_src = pmc_traffic(dom, workload if crop is None else "%s_%dx%d" % (workload, crop[0], crop[1]))
                    roofline = {"kernel": dom, "bound": "mfma", "achieved": round(ach, 2), "peak": peak,
                                "unit": "TFLOP/s", "frac": round(ach / peak, 4), "traffic": traffic,
                                "traffic_unit": "HBM-side bytes per launch", "traffic_source": traffic_src,
                                "algorithmic_bytes_per_launch": round(algo_bytes[dom] / n) if dom in algo_bytes else None,
                                "avg_launch_us": round(1e3 * t_ms / n, 2), "launches": n,
                                "flops_per_launch": fl / n,
                                "measured": "HIP events around every launch, %s" %
                                            ("eager pass after the graph-replayed timed region" if use_graph
                                             else "inside the timed region")}
            if is_db:
                metric_name = "training images/sec, DB detector (deformable ResNet-50 + SegDetector) 640x640, batch %d per GPU" % bsz
                workload_name = ("DB text detector training step (BASELINE.json configs[4]): deformable_resnet50 (13 "
                                 "DCNv2 layers) + SegDetector(adaptive, k=50) + L1BalanceCELoss, SGD momentum 0.9, "
                                 "640x640 images")
                fwd_flops = 127.2e9  # 94.03 backbone (24.54 of it DCN GEMMs) + 33.20 head
            elif workload == "fpn_attention":
                metric_name = "training images/sec, ResNet50-FPN + attention decoder 64x256 crops, batch %d per GPU" % bsz
                workload_name = ("ResNet50-FPN + attention GRU decoder training step (BASELINE.json configs[3]): 64x256 "
                                 "crops, 32 decode steps, %s, Adam" %
                                 ("teacher forcing by a coin per step (gt_as_output=None, the YAML default)" if random_coins
                                  else "teacher forcing fixed (gt_as_output)"))
                fwd_flops = 17.25e9  # 5.01 backbone + 10.97 decoder conv encoder + 1.27 decode loop
            elif workload == "res50ppm":
                ch, cw = crop or (32, 128)
                metric_name = "training images/sec, ResNet50-PPM-2D-CTC %dx%d crops, batch %d per GPU" % (ch, cw, bsz)
                workload_name = ("ResNet50-dilated-PPM + 2D-CTC training step (BASELINE.json configs[2]): %dx%d crops, "
                                 "T=%d H=%d C=38, Adam" % (ch, cw, cw // 8, ch // 8))
                fwd_flops = 6.02e9 * (ch * cw) / (32.0 * 128.0)  # 6.02 GFLOP forward per 32x128 image
            else:
                metric_name = "training images/sec, CRNN-CTC 32x128 crops, batch %d per GPU" % bsz
                workload_name = "CRNN + 1D-CTC training step (BASELINE.json configs[1]): 32x128 crops, T=33, C=38, Adam"
                fwd_flops = 1.80e9
            out = {
                "metric": metric_name,
                "value": round(images / elapsed, 1), "unit": "images/s", "n_gpus": world, "steps": steps,
                "warmup": warmup, "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": scaling,
                "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
                "config": {"workload": workload_name, "global_batch": bsz * world,
                           "per_gpu_batch": bsz, "parallelism": "dp%d" % world,
                           "launch": ("hipGraph replay" if not distributed else ddp_launch) if use_graph
                           else ("eager" if not distributed else "eager, apex-style DDP shim (bucketed, overlapped)"),
                           "train_flops_per_image": 3 * fwd_flops, **({"tuning": args.set} if args.set else {})},
                "final_loss": final_loss,
                "roofline": roofline,
                "kernels": kernels,
            }
            shim = net if hasattr(net, "last_backward") else None
            if shim is not None and shim.last_backward:
                # all-reduces the last recorded backward issued (= all-reduce nodes of the captured graph in capture mode)
                out["config"]["ddp"] = dict(shim.last_backward)
            step_tflops = 3 * fwd_flops * bsz / (ms * 1e-3) / 1e12
            out["step_tflops_per_gpu"] = round(step_tflops, 2)
            out["host_enqueue_ms_per_step"] = round(1e3 * host_enqueue / steps, 3)
            if world == 1 and with_cpu:
                out["cpu_baseline"] = cpu_baseline(workload, budget_s=20.0 if workload == "crnn" else 12.0, crop=crop)
            else:
                out["cpu_baseline"] = None
        else:
            out = None
        return out

    out = measure(args.workload, args.steps, args.warmup, args.full and not args.no_cpu_baseline, dump_dir=args.dump_outputs)
    if args.full and out is not None and world == 1 and not distributed and args.workload == "crnn" and not args.no_secondary:
        # the other three published configurations ride along in the default single-GPU line: BASELINE.json north_star
        # target #2 (configs[2], also kept under the round-1..3 key `secondary`), configs[3] and configs[4]; each with its own
        # roofline block and CPU baseline
        out["secondaries"] = []
        for wl, crop, coins in (("res50ppm", None, None), ("fpn_attention", None, "fixed"), ("db", None, None),
                                ("res50ppm", (64, 256), None), ("fpn_attention", None, "random")):
            sec = measure(wl, min(args.steps, 10), min(args.warmup, 3), not args.no_cpu_baseline and coins != "random", crop=crop,
                          coins=coins)
            for k in ("n_gpus", "higher_is_better", "scaling", "vs_baseline", "data"):
                sec.pop(k, None)
            sec["workload"] = (wl if crop is None else "%s_%dx%d" % (wl, crop[0], crop[1])) + ("_random_coins" if coins == "random" else "")
            out["secondaries"].append(sec)
        out["secondary"] = out["secondaries"][0]
    if args.full and world > 1 and args.scaling == "weak" and not args.no_strong:
        # N > 1: the same line also carries the STRONG-scaling measurement -- the workload's global batch (256 crops) sharded
        # over the ranks as the reference's loader does (data/data_loader.py:40-48) -- whichever --scaling the driver passed
        # (VERDICT r4 item 9).  A second model / optimizer / captured step in the same process; a failure is reported, not fatal.
        try:
            import gc
            gc.collect()
            torch.cuda.synchronize()
            strong = measure(args.workload, args.steps, args.warmup, False, scaling="strong")
            if out is not None:
                out["strong"] = {k: strong[k] for k in ("metric", "value", "unit", "ms_per_step", "scaling", "config",
                                                         "final_loss", "host_enqueue_ms_per_step") if k in strong}
        except Exception as e:  # noqa: BLE001
            if out is not None:
                out["strong"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if distributed:
        torch.cuda.synchronize()
        dist.barrier()     # every rank is past its timed region and its part of the result
    emit_last_line(json.dumps(out) if out is not None else None)
    if distributed:
        # Leave WITHOUT tearing the process group down: on this ROCm 7.0 / RCCL 2.26 stack destroy_process_group() -- and the
        # communicator's destructor at interpreter exit -- intermittently aborts the process (SIGABRT in ProcessGroupNCCL's
        # shutdown, seen in tests/test_ddp_gpu.py in round 4).  The result line is out and every rank has passed the barrier:
        # a crash here would only turn a finished measurement into a failed run.
        sys.stderr.flush()
        os._exit(0)


if __name__ == "__main__":
    main()
