#!/usr/bin/env python3
"""Benchmark of the hot path: frame-pairs/sec for flow + warp + mask at 512x768 on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]

One "step" = one pass of the hot path over one batch of synthetic input per GPU: B frames
(default 64 = BASELINE.json configs[2]/[3], "64-frame 512x768 clip ... HBM-resident cost volumes")
against one shared key frame: RAFT dense flow (fp32, 20 iterations, frame -> key frame) -> bilinear
backward warp of the AI key frame -> low-confidence inpaint mask (conf < 0.95, 7x7 ellipse dilate).
Inputs are resident in HBM before the timed region.  N > 1: one process per GPU (torchrun), frames
sharded frame-parallel (weak scaling, B per GPU), one RCCL broadcast of the key frame pair per step,
no other collective.

Prints ONE JSON line (rank 0) with the driver's contract fields plus
  "roofline":     the dominant kernel family (fp32-MFMA implicit-GEMM convolutions) measured live
                  with HIP events on the launch stream inside the timed region,
  "kernels":      the same measurement for the HBM-bound kernels (correlation volume, lookup,
                  upsample, warp, mask) against the 8 TB/s HBM peak.
A plain run stops there: set-up, warm-up, the timed steps, --dump-outputs and the line.  --full adds every
measurement beyond the headline, each after the timed region (the --no-* switches leave single ones out):
  "verified":     three pairs of the last timed step against the CPU oracle in fp32 and float64,
  "cpu_baseline": the CPU oracle (a port; the reference's Python cannot travel to the GPU box) timed
                  on the host cores on a bounded sample of the same workload,
  "single_pair":  BASELINE.json configs[1] (one 512x768 pair) latency/throughput,
  "batch_sweep":  the batches in between (1, 4, 16, 64 frames per call),
  "workspace_pipeline": the path end to end over a PNG workspace (`pipeline.ClipPipeline.run`: decode -> H2D -> flow both ways ->
                  warp + mask -> SD-inpaint inputs -> render -> D2H -> encode) against the same calls on resident frames, with the
                  host CPU-seconds per frame and the one-batch-per-rank share of BASELINE configs[3]; never `value`,
  "raft2_as_written", "sd_handoff_1024", "kernels.corr_volume_gemm_split", "fast_mode", "split3_mode": the
                  other configurations and precisions, on the same clip.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W = 768, 512                 # "512x768" = W x H (SURVEY conventions)
ITERS = 20
HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: 8.0 TB/s spec
HBM_ACHIEVABLE_GBS = 6300.0     # same guide: what a well-formed streaming kernel reaches on this part (~0.79 of the spec)
MFMA_F32_PEAK_TFLOPS = 157.3    # v_mfma_f32_32x32x2_f32 dense peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # v_mfma_f32_32x32x16_bf16 dense peak (same guide; AMD's 5 PF headline includes 2:1 sparsity)


# ----------------------------------------------------------------------------------------------
# algorithmic work per pair, used as roofline numerators
# ----------------------------------------------------------------------------------------------
def conv_flops(hw, cin, cout, kh, kw):
    return 2.0 * hw * cin * cout * kh * kw


def encoder_flops(H, W):
    f = conv_flops((H // 2) * (W // 2), 3, 64, 7, 7)
    hw2, hw4, hw8 = (H // 2) * (W // 2), (H // 4) * (W // 4), (H // 8) * (W // 8)
    f += 4 * conv_flops(hw2, 64, 64, 3, 3)
    f += conv_flops(hw4, 64, 96, 3, 3) + 3 * conv_flops(hw4, 96, 96, 3, 3) + conv_flops(hw4, 64, 96, 1, 1)
    f += conv_flops(hw8, 96, 128, 3, 3) + 3 * conv_flops(hw8, 128, 128, 3, 3) + conv_flops(hw8, 96, 128, 1, 1)
    f += conv_flops(hw8, 128, 256, 1, 1)
    return f


def update_flops(H, W, with_mask):
    n = (H // 8) * (W // 8)
    f = conv_flops(n, 324, 256, 1, 1) + conv_flops(n, 256, 192, 3, 3) + conv_flops(n, 2, 128, 7, 7)
    f += conv_flops(n, 128, 64, 3, 3) + conv_flops(n, 256, 126, 3, 3)
    f += 6 * conv_flops(n, 384, 128, 1, 5)
    f += conv_flops(n, 128, 256, 3, 3) + conv_flops(n, 256, 2, 3, 3)
    if with_mask:
        f += conv_flops(n, 128, 256, 3, 3) + conv_flops(n, 256, 576, 1, 1)
    return f


def algorithmic_work(H, W, B, shared_key=True):
    """FLOPs of all convolutions and bytes of the HBM-bound kernels for one step of B pairs."""
    n = (H // 8) * (W // 8)
    n_enc = (B + 1) if shared_key else 2 * B          # fnet images
    conv = (n_enc + B) * encoder_flops(H, W)          # + cnet on every frame
    conv += B * (ITERS * update_flops(H, W, False) + (update_flops(H, W, True) - update_flops(H, W, False)))
    lvl = [n * ((H // 8) >> l) * ((W // 8) >> l) * 4.0 for l in range(4)]      # bytes of each pyramid level per pair
    pyr = sum(lvl)
    # level 1 leaves the volume GEMM's epilogue when it is tiled by whole 4x8 blocks (corr.hip: ofx_corr_volpool_ok);
    # the pooling kernel then starts from level 1 instead of re-reading level 0
    fused = (H // 8) % 8 == 0 and (W // 8) % 16 == 0
    return {
        "conv_flops": conv,
        # what the kernels actually execute: the context (`inp`) third of the six GRU convolutions is
        # loop-invariant and evaluated once per pair instead of once per iteration
        "conv_flops_executed": conv - B * (ITERS - 1) * 6 * conv_flops(n, 128, 128, 1, 5),
        "volume_flops": B * 2.0 * n * n * 256,
        "volume_bytes": B * (n * 256 * 4.0 + lvl[0] + (lvl[1] if fused else 0.0)) + (1 if shared_key else B) * n * 256 * 4.0,   # GEMM: read fmaps, write level 0 (+ level 1)
        "pool_bytes": B * ((lvl[1] + lvl[2] + lvl[3]) if fused else pyr),                                # read level 1 (or 0), write the levels below
        "pool_reread_bytes": B * (lvl[1] if fused else lvl[0]),                                         # the level the pooling kernel reads back
        "lookup_bytes": B * n * (400 * 4.0 + 324 * 4.0 + 8.0),                                          # per launch
        "upsample_bytes": B * (n * 576 * 4.0 + n * 8.0 + H * W * 8.0),
        "warp_bytes": B * (H * W * 8.0 + H * W * 3.0) + H * W * 3.0,
        # upsample with the warp inside (one kernel): mask logits + coords in, flow_up + warped out, the key frame once -- the union of
        # the two kernels' algorithmic bytes minus the flow re-read that no longer happens
        "upsample_warp_bytes": B * (n * 576 * 4.0 + n * 8.0 + H * W * 8.0 + H * W * 3.0) + H * W * 3.0,
        "mask_bytes": B * (H * W * 4.0 + H * W * 1.0),
    }


# ----------------------------------------------------------------------------------------------
# synthetic clip
# ----------------------------------------------------------------------------------------------
def make_clip(B, H, W, device, rank=0):
    g = torch.Generator(device="cpu").manual_seed(1234)
    noise = torch.rand((1, 3, H, W), generator=g)
    key = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(noise, (4, 4, 4, 4), mode="reflect"), 9, 1)
    key = (key - key.min()) / (key.max() - key.min())
    key = key.to(device)
    ys, xs = torch.meshgrid(torch.arange(H, device=device, dtype=torch.float32),
                            torch.arange(W, device=device, dtype=torch.float32), indexing="ij")
    # the sensor noise has a seeded generator of its own: torch's default one can start from a different seed in every process,
    # and the inputs must be the same from run to run
    gn = torch.Generator(device=device).manual_seed(5678 + rank)
    frames = []
    for t in range(B):
        ph = 0.37 * (t + 1 + 64 * rank)
        fx = 8.0 * torch.sin(2 * math.pi * ys / H + ph) * torch.cos(2 * math.pi * xs / W)
        fy = 6.0 * torch.cos(2 * math.pi * xs / W + 0.5 * ph)
        gx = 2 * (xs + fx) / (W - 1) - 1
        gy = 2 * (ys + fy) / (H - 1) - 1
        fr = torch.nn.functional.grid_sample(key, torch.stack([gx, gy], -1)[None], mode="bilinear", padding_mode="border",
                                             align_corners=True)
        fr = fr * 255 + 2.0 * torch.randn(fr.shape, device=device, generator=gn)
        frames.append(fr.clamp(0, 255).round().to(torch.uint8)[0].permute(1, 2, 0))
    frames = torch.stack(frames).contiguous()
    key_u8 = (key[0] * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    key_ai = (255 - key_u8).contiguous()
    gc = torch.Generator(device="cpu").manual_seed(4321 + rank)
    cn = torch.randn((B, 1, H // 16, W // 16), generator=gc)
    conf = torch.sigmoid(torch.nn.functional.interpolate(cn, size=(H, W), mode="bilinear", align_corners=False)[:, 0] * 2.0 + 3.6)
    conf[:, ::37, ::29] = 0.95          # planted exact-threshold values
    conf[:, 5::41, 3::31] = 0.9
    return frames, key_u8, key_ai, conf.to(device).contiguous()


# ----------------------------------------------------------------------------------------------
def usable_cores() -> int:
    """Cores this process may actually use: affinity mask capped by the cgroup CPU quota (a GPU box can
    report hundreds of CPUs while the container is limited to a few -- oversubscribing torch's thread pool
    there is catastrophically slow)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()
            if q != "max":
                n = min(n, max(1, int(math.ceil(int(q) / int(p)))))
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, int(math.ceil(q / p))))
        except Exception:
            pass
    return max(1, n)


def pick_cpu_threads() -> int:
    """Micro-benchmark a representative convolution at a few thread counts and keep the fastest."""
    cap = usable_cores()
    cands = sorted({min(cap, c) for c in (cap, 64, 32, 16, 8)})
    x = torch.randn(1, 128, 96, 64)
    w = torch.randn(128, 128, 3, 3)
    best, best_t = cands[0], float("inf")
    for c in cands:
        torch.set_num_threads(c)
        torch.nn.functional.conv2d(x, w, padding=1)
        t0 = time.perf_counter()
        for _ in range(5):
            torch.nn.functional.conv2d(x, w, padding=1)
        dt = time.perf_counter() - t0
        if dt < best_t:
            best, best_t = c, dt
        if dt > 2.0:          # pathological: stop probing larger pools
            break
    return best


def verify_against_oracle(path):
    """Three pairs of the timed batch (first, middle, last frame; key frame, AI key frame, confidence and the GPU's flow / warped /
    mask for them, written by the bench process after the timed region) against the CPU oracle -- and against the SAME oracle
    evaluated in float64, the yardstick that says how much of the distance is the fp32 CPU oracle's own rounding."""
    import numpy as np
    from oracle import mask_oracle, raft_oracle, warp_oracle
    z = np.load(path)
    sd = raft_oracle.init_state_dict(0)
    sd64 = raft_oracle.to_float64(sd)
    b = torch.from_numpy(z["key"]).permute(2, 0, 1)[None].float()
    t0 = time.time()
    pairs = []
    epe = lambda d: float(np.sqrt((d * d).sum(-1)).mean())
    for i, idx in enumerate(z["index"].tolist()):
        a = torch.from_numpy(z["frame"][i]).permute(2, 0, 1)[None].float()
        _, up = raft_oracle.raft_forward(sd, a, b, iters=ITERS)
        ref = up[0].permute(1, 2, 0).contiguous().numpy()
        d = z["flow"][i] - ref
        wref = warp_oracle.warp_frame(z["key_ai"], z["flow"][i], mode=str(z["warp_mode"]))
        wd = np.abs(wref.astype(np.int32) - z["warped"][i].astype(np.int32))
        mref, _ = mask_oracle.generate_mask(z["conf"][i], z["conf"][i].copy(), 0.95, 7)
        rec = {"pair": int(idx), "flow_epe_px": epe(d), "flow_max_err_px": float(np.sqrt((d * d).sum(-1)).max()),
               "warp_max_abs_diff_u8": int(wd.max()), "warp_frac_pixels_differing": float((wd > 0).mean()),
               "mask_bit_exact": bool(np.array_equal(mref, z["mask"][i]))}
        for mode in ("bf16x6", "bf16x3"):       # the same pair with ONLY the correlation volume in split-bf16 form
            if "flow_vol_" + mode in z.files:
                rec["volume_" + mode + "_epe_px"] = epe(z["flow_vol_" + mode][i] - ref)
        if time.time() - t0 < 150:              # float64 yardstick (bounded: the child process has a hard time limit)
            _, up64 = raft_oracle.raft_forward(sd64, a.double(), b.double(), iters=ITERS)
            r64 = up64[0].permute(1, 2, 0).contiguous().numpy()
            rec["gpu_epe_vs_f64_px"] = epe(z["flow"][i].astype(np.float64) - r64)
            rec["cpu_fp32_oracle_epe_vs_f64_px"] = epe(ref.astype(np.float64) - r64)
            for mode in ("bf16x6", "bf16x3"):
                if "flow_vol_" + mode in z.files:
                    rec["volume_" + mode + "_epe_vs_f64_px"] = epe(z["flow_vol_" + mode][i].astype(np.float64) - r64)
        pairs.append(rec)
    bn_batch = None
    if "flow_bn_batch" in z.files:          # the RAFT_2-as-written network (cnet_norm='batch') on pair 0 of the batch
        a = torch.from_numpy(z["frame"][0]).permute(2, 0, 1)[None].float()
        _, upb = raft_oracle.raft_forward(sd, a, b, iters=ITERS, cnet_norm="batch")
        d = z["flow_bn_batch"][0] - upb[0].permute(1, 2, 0).contiguous().numpy()
        bn_batch = {"pair": int(z["index"][0]), "flow_epe_px": epe(d), "flow_max_err_px": float(np.sqrt((d * d).sum(-1)).max())}
    worst = max(pairs, key=lambda r: r["flow_epe_px"])
    out = dict(worst)
    if bn_batch:
        out["raft2_as_written"] = bn_batch
    out.update({"pairs": pairs, "mask_bit_exact": all(r["mask_bit_exact"] for r in pairs),
                "warp_max_abs_diff_u8": max(r["warp_max_abs_diff_u8"] for r in pairs), "oracle_s": round(time.time() - t0, 2)})
    return out


def cpu_baseline(budget_s=15.0, max_pairs=24, verify=None):   # a bounded sample: ~15-20 s of CPU work
    """The CPU oracle (port of the reference's path) on the host cores: flow + warp + mask per pair."""
    from oracle import mask_oracle, raft_oracle, warp_oracle
    # A FIXED rule, so that the baseline is comparable from round to round: every usable core up to 16 (the oracle's convolutions stop
    # scaling there; rounds 1-4 ran 16 threads, round 5's per-run probe picked 8 on the same boxes and the figure moved 1.17 -> 0.89 for
    # that reason alone).  `pick_cpu_threads` stays as a diagnostic.
    threads = min(usable_cores(), 16)
    torch.set_num_threads(threads)
    out = {}
    if verify:
        out["verified"] = verify_against_oracle(verify)
    sd = raft_oracle.init_state_dict(0)
    frames, key, key_ai, conf = make_clip(max_pairs, H, W, "cpu")
    done, t0 = 0, time.time()
    while done < max_pairs and (done == 0 or time.time() - t0 < budget_s):
        a = frames[done].permute(2, 0, 1)[None].float()
        b = key.permute(2, 0, 1)[None].float()
        _, up = raft_oracle.raft_forward(sd, a, b, iters=ITERS)
        flow = up[0].permute(1, 2, 0).contiguous().numpy()
        warp_oracle.warp_frame(key_ai.numpy(), flow, mode="bilinear")
        mask_oracle.generate_mask(conf[done].numpy(), conf[done].numpy().copy(), 0.95, 7)
        done += 1
    dt = time.time() - t0
    out.update({"value": done / dt, "unit": "pairs/s", "cores": threads, "threads": threads, "usable_cores": usable_cores(), "kind": "port",
                "sample": f"{done} pair(s) 512x768, RAFT {ITERS} iters fp32 + bilinear warp + mask, torch-CPU oracle, {dt:.1f} s"})
    return out


def flush_c_stdio():
    """RCCL / the HIP runtime write banner lines through C stdio; when stdout is a pipe they sit in a buffer until the
    process exits and would land AFTER rank 0's result line (on any rank: torchrun merges the streams)."""
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start N ranks ourselves (one process per GPU
    under torch.distributed.run, RCCL rendezvous on 127.0.0.1) instead of measuring one GPU under a label that says N."""
    have = 0 if args.stub_step else torch.cuda.device_count()
    if have < args.gpus and not args.stub_step:
        print(f"bench.py: --gpus {args.gpus} asked for but only {have} HIP device(s) are visible; refusing to measure "
              f"fewer GPUs than requested", file=sys.stderr)
        sys.exit(2)
    import socket
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # a child process, not os.exec*: counting the devices has started the GPU runtime in this one
    import subprocess
    sys.exit(subprocess.run(cmd).returncode)


def make_step(eng, frames, key, key_ai, conf, warp_mode="bilinear", separate_warp=False):
    """The timed step, importable (tests/test_gpu_raft.py runs exactly this on the headline batch): the product's own
    `clip.FrameSynthesizer` -- what `pipeline.ClipPipeline` and `clip.process_clip` run -- fed by the flow network alone with the clip's
    synthetic confidence: frame -> key frame flow (shared image2), the AI key frame warped inside the convex upsample when the warp is
    bilinear, the confidence-threshold mask; plus the path's only exchange, the key-frame broadcast (a no-op on one rank).
    Returns step() -> (flow f32[B,H,W,2], warped u8 [B,H,W,3], mask u8 [B,H,W])."""
    from sd_animation_optical_flow_amd import clip
    synth = clip.FrameSynthesizer(engine=eng, warp_mode=warp_mode, thres=0.95, ksize=7, iters=ITERS, fuse_warp=not separate_warp)

    def step():
        clip.broadcast_keyframe([key, key_ai], src=0)
        return synth(frames, key, key_ai, confidence=conf)
    return step


def workspace_end_to_end(args, dist, dev, rank, world):
    """`--workspace`: the rank-parallel END-TO-END mode (SURVEY 8e names a rank's decode / H2D / encode as the limit of the 8-GPU
    scaling, and the resident-frame `value` cannot show it).  One shared PNG workspace of `world` key-frame segments x `--ws-segment`
    frames (BASELINE configs[3] at world = 8: 8 x 64 frames of 512x768) written by rank 0; every rank then runs the product's own
    `pipeline.ClipPipeline.run` on its share of the plan -- PNG decode -> H2D -> flow both ways + forward-backward confidence -> warp +
    mask -> SD-inpaint inputs -> render -> D2H -> PNG encode -- between two barriers.  Reported per rank: frames, wall seconds,
    end-to-end frames/s, host CPU-seconds per frame; for the job: total frames / MAX wall over the ranks.  Secondary keys only: `value`
    stays the resident-frame number.  `--stub-step` swaps the compute step for CPU arithmetic (the gloo test of the rank plumbing)."""
    import shutil
    import tempfile
    import numpy as np
    from sd_animation_optical_flow_amd import clip, pipeline
    from sd_animation_optical_flow_amd.workspace import VideoData
    stub = args.stub_step
    h, w = (16, 24) if stub else (H, W)
    seg = max(2, int(args.ws_segment))
    n_seg = max(1, world)
    n = n_seg * seg
    flags = [i % seg == 0 for i in range(n)]
    root = [None]
    if rank == 0:
        root[0] = tempfile.mkdtemp(prefix="ofx_bench_ws_")
        if stub:
            rng = np.random.default_rng(3)
            clip_frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]
        else:
            frames, key, _, _ = make_clip(seg - 1, h, w, dev)
            clip_frames = []
            for sgi in range(n_seg):                              # segment: its key frame, then seg - 1 frames that move against it
                clip_frames.append(torch.roll(key, shifts=17 * sgi, dims=1).cpu().numpy())
                clip_frames += [f for f in torch.roll(frames, shifts=17 * sgi, dims=2).cpu().numpy()]
            del frames, key
        VideoData(clip_frames, (w, h), root[0])
        del clip_frames
    if dist is not None:
        dist.broadcast_object_list(root, src=0)
    try:
        video = VideoData(None, (w, h), root[0])
        if stub:
            class StubPipe(pipeline.ClipPipeline):
                def process_batch(self, key_raw, key_ai, raws, ids, key_index):
                    return [pipeline.FramePacket(t, key_index, torch.zeros(1), torch.zeros(1), (raws[k] // 2 + key_ai // 2).to(torch.uint8),
                                                 ((raws[k][..., 0] > 128).to(torch.uint8) * 255), {}) for k, t in enumerate(ids)]
            pipe = StubPipe(algo=None, render=lambda pkt, raw: torch.where(pkt.mask[..., None] > 0, raw, pkt.warped), batch=4,
                            device=torch.device("cpu"), io_threads=1, edge_batch=2)
        else:
            from sd_animation_optical_flow_amd import pdcnet_of
            pipe = pipeline.ClipPipeline(pdcnet_of.PDCNetPlus("random:0", device=dev), batch=args.batch, warp_mode="bilinear", thres=0.95, ksize=7)
        plan = clip.plan_segments(flags, world)
        mine = sum(len(p.frames[rank]) for p in plan) + sum(1 for p in plan if p.owner == rank)
        sync = (lambda: None) if stub else torch.cuda.synchronize

        def once():
            if dist is not None:
                dist.barrier()
            sync()
            c0, t0 = time.process_time(), time.perf_counter()
            pipe.run(video, flags)
            sync()
            return time.perf_counter() - t0, time.process_time() - c0
        if not stub:
            once()                                               # warm-up: workspaces, thread pools, pinned buffers, page cache
        dt, cpu = once()
        rec = {"rank": rank, "frames": mine, "wall_s": round(dt, 4), "end_to_end_fps": round(mine / dt, 2) if mine else 0.0,
               "host_cpu_s_per_frame": round(cpu / mine, 5) if mine else None, "io_threads": pipe.io_threads}
        recs = [rec]
        if dist is not None:
            recs = [None] * world
            dist.all_gather_object(recs, rec)
            dist.barrier()
        if rank != 0:
            return None
        wall = max(r["wall_s"] for r in recs)
        ok = all(video.generated(i) for i in range(n))
        return {"workload": f"{n}-frame {min(h, w)}x{max(h, w)} PNG workspace shared by the ranks, {n_seg} key-frame segments x {seg} frames "
                            f"(BASELINE configs[3] at 8 ranks), ClipPipeline.run per rank on its plan share, PNG in -> PNG out",
                "ranks": world, "frames": n, "every_frame_written": ok, "max_wall_s": wall, "job_end_to_end_fps": round(n / wall, 2),
                "per_rank": recs, "usable_cores": usable_cores(), "compute": "cpu stub" if stub else "hip",
                "broadcasts": sum(1 for p in plan if p.needs_broadcast),
                "note": "secondary: `value` times resident frames.  A curve over N exists only where the driver ran this command on N "
                        "devices; no multi-GPU run was taken from the build sessions (one device per box)"}
    finally:
        if dist is not None:
            dist.barrier()
        if rank == 0 and root[0]:
            shutil.rmtree(root[0], ignore_errors=True)


DUMP_LIMIT_BYTES = 64 * 10**6


def dump_outputs(outdir, last, seed=0):
    """What the last timed step returned -- flow f32 [B,H,W,2], warped u8 [B,H,W,3], mask u8 [B,H,W] -- as float32 .npy files in
    `outdir`.  All B frames when they fit in DUMP_LIMIT_BYTES; otherwise a seeded choice of whole frames (`frame_index.npy`) and, for
    every frame of the batch, the same seeded pixel positions (`*_pixels.npy`, positions in `pixel_yx.npy`)."""
    import numpy as np
    flow, warped, mask = last
    B, Hh, Ww = mask.shape
    per_frame = 4 * Hh * Ww * (flow.shape[-1] + warped.shape[-1] + 1)
    g = torch.Generator().manual_seed(seed)
    if B * per_frame <= DUMP_LIMIT_BYTES:
        frames = torch.arange(B)
        pix = None
    else:
        n_pix = min(Hh * Ww, 4096)
        budget = DUMP_LIMIT_BYTES - B * n_pix * per_frame // (Hh * Ww) - 8 * (n_pix * 2 + B)
        frames = torch.randperm(B, generator=g)[:max(1, budget // per_frame)].sort().values
        pix = torch.randperm(Hh * Ww, generator=g)[:n_pix].sort().values
    os.makedirs(outdir, exist_ok=True)
    out = {"frame_index": frames.double()}
    for name, t in (("flow", flow), ("warped", warped), ("mask", mask)):
        out[name] = t[frames.to(t.device)].float()
        if pix is not None:
            out[name + "_pixels"] = t.reshape(B, Hh * Ww, *t.shape[3:])[:, pix.to(t.device)].float()
    if pix is not None:
        out["pixel_yx"] = torch.stack([pix // Ww, pix % Ww], -1).double()
    for name, t in out.items():
        np.save(os.path.join(outdir, name + ".npy"), t.cpu().numpy())
    return sorted(out)


def stub_step_factory(dev):
    """CPU stand-in for the hot path (hidden --stub-step): lets the world_size-2 gloo test drive every line of the
    rank plumbing (init, key-frame broadcast, barrier, timed loop, MAX all-reduce, one JSON line) without a GPU."""
    from sd_animation_optical_flow_amd import clip
    key = torch.zeros((8, 8, 3), dtype=torch.uint8, device=dev)
    key_ai = torch.zeros_like(key)

    def step():
        clip.broadcast_keyframe([key, key_ai], src=0)
        time.sleep(0.01)
        return None
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU per step")
    ap.add_argument("--warp-mode", default="bilinear", choices=["bilinear", "bicubic", "cv2_cubic"])
    ap.add_argument("--separate-warp", action="store_true", help="upsample and warp as two kernels (default: the warp runs inside the convex upsample)")
    ap.add_argument("--no-prof", action="store_true", help="do not bracket launches with HIP events")
    ap.add_argument("--prof-all-steps", action="store_true", help="bracket the launches of every timed step with HIP events (default: the last step only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle check of one sampled pair")
    ap.add_argument("--no-single", action="store_true")
    ap.add_argument("--no-handoff", action="store_true", help="skip the 1024x1024 SD-inpaint hand-off timing (config #5's non-generative half)")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16x3", "bf16x6"],
                    help="matrix-core arithmetic of the timed run (fp32 = the reference's; bf16x3 = opt-in split-bf16 fast mode)")
    ap.add_argument("--no-fast", action="store_true", help="skip the secondary bf16x3 measurement")
    ap.add_argument("--no-volsplit", action="store_true", help="skip the secondary lines with ONLY the correlation volume in split-bf16 form")
    ap.add_argument("--no-sweep", action="store_true", help="skip the small-batch sweep (B = 1, 4, 16 frames per call)")
    ap.add_argument("--no-pipeline", action="store_true", help="skip the workspace pipeline measurement (PNG in -> ClipPipeline.run -> PNG out)")
    ap.add_argument("--cpu-baseline-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--verify-npz", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--verify-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--stub-step", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--workspace", action="store_true", help="also run the rank-parallel END-TO-END mode: every rank runs ClipPipeline.run "
                    "on its share of one shared PNG workspace (secondary keys under `workspace_ranks`; `value` is unchanged)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed (flow, warped frame, mask; float32 .npy, <= 64 MB) into DIR")
    ap.add_argument("--ws-segment", type=int, default=64, help="frames per key-frame segment of the --workspace mode (one segment per rank)")
    ap.add_argument("--full", action="store_true", help="after the timed steps, also run every secondary measurement: oracle check, CPU "
                    "baseline, single pair, batch sweep, hand-off, other precisions, workspace pipeline (the --no-* switches apply here)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if not args.full:
        # a plain run measures the headline alone: every block after the timed region is --full's
        args.no_verify = args.no_cpu_baseline = args.no_single = args.no_sweep = True
        args.no_handoff = args.no_fast = args.no_volsplit = args.no_pipeline = True
    if args.cpu_baseline_only:
        print(json.dumps(cpu_baseline(verify=args.verify_npz)))
        return
    if args.verify_only:
        torch.set_num_threads(pick_cpu_threads())
        print(json.dumps({"verified": verify_against_oracle(args.verify_npz)}))
        return

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)                    # does not return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # a launcher that started a different number of ranks than the command line names: the line would be mislabelled
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; start it as `python bench.py --gpus N` or under "
              f"torch.distributed.run with --nproc-per-node N", file=sys.stderr)
        sys.exit(2)
    backend = "gloo" if args.stub_step else "nccl"
    # OFX_BENCH_FORCE_DIST=1 exercises the RCCL code path (init, broadcast, barrier, all-reduce) on one rank
    use_dist = world > 1 or (os.environ.get("OFX_BENCH_FORCE_DIST") == "1" and "MASTER_PORT" in os.environ)
    if not args.stub_step and torch.cuda.device_count() <= local_rank:
        print(f"bench.py: rank {rank} needs HIP device {local_rank} but only {torch.cuda.device_count()} are visible", file=sys.stderr)
        sys.exit(2)
    dev = torch.device("cpu") if args.stub_step else torch.device("cuda", local_rank if use_dist else 0)
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.stub_step:
            dist.init_process_group(backend)
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend, device_id=dev)
    else:
        dist = None
        if not args.stub_step:
            torch.cuda.set_device(0)
    n_gpus = world
    sync = (lambda: None) if args.stub_step else torch.cuda.synchronize

    B = args.batch
    if args.stub_step:
        step = stub_step_factory(dev)
        ops = None
    else:
        from sd_animation_optical_flow_amd import clip, ops
        from sd_animation_optical_flow_amd.raft import RaftEngine
        from sd_animation_optical_flow_amd.weights import random_state_dict
        eng = RaftEngine(random_state_dict(0), dev, precision=args.precision)
        frames, key, key_ai, conf = make_clip(B, H, W, dev, rank)

        step = make_step(eng, frames, key, key_ai, conf, args.warp_mode, args.separate_warp)

    def barrier():
        if dist is not None:
            dist.barrier()
        sync()

    # how many ranks the collective library actually sees (RCCL's own count, not the environment's)
    ranks_seen = 1
    if dist is not None:
        one = torch.ones((1,), device=dev, dtype=torch.float32)
        dist.all_reduce(one)
        ranks_seen = int(round(float(one.item())))

    for _ in range(args.warmup):
        step()
    prof = not args.no_prof and ops is not None
    barrier()
    flush_c_stdio()                          # every rank: library banners out before anybody prints a result
    # HIP events bracket every launch of the LAST timed step only (per layer: "family:layer"; families are re-aggregated below).
    # Two events per launch cost ~1 % of the step (measured round 4: 327.98 ms/step without, 331.31 with, 5 steps each) -- a
    # command-processor barrier before and after each of ~450 kernels -- so the K - 1 steps before it run as the product runs them;
    # the roofline's per-kernel durations are the averages over that step's launches (255 convolutions).  --prof-all-steps brackets
    # every step (what rounds 1-3 did).
    prof_steps = 0
    last = None
    t0 = time.perf_counter()
    for i in range(args.steps):
        if prof and (args.prof_all_steps or i == args.steps - 1):
            ops.prof_enable(2)               # a host-side flag: nothing is synchronised between the steps
            prof_steps += 1
        last = step()
    barrier()
    elapsed = time.perf_counter() - t0
    layers = {}
    if prof:
        layers = ops.prof_collect()
        ops.prof_enable(False)
    dumped = None
    if args.dump_outputs and rank == 0 and last is not None:
        dumped = dump_outputs(args.dump_outputs, last)
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ws_ranks = None
    if args.workspace:
        ws_ranks = workspace_end_to_end(args, dist, dev, rank, world)
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        flush_c_stdio()
        return

    ms_per_step = 1e3 * elapsed / args.steps
    value = n_gpus * B * args.steps / elapsed
    work = algorithmic_work(H, W, B)
    out = {
        "metric": "frame-pairs/sec (flow+warp+mask) at 512x768",
        "value": round(value, 3), "unit": "pairs/s", "n_gpus": n_gpus, "ranks_seen": ranks_seen, "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32" if args.precision == "fp32" else args.precision + " (fp32 operands split into bf16 pieces, fp32 accumulate)", "data": "synthetic",
        "config": {"workload": f"BASELINE configs[2]: {B}-frame 512x768 clip per GPU vs one shared key frame, RAFT {ITERS} iters "
                               f"fp32 + {args.warp_mode} warp + mask(conf<0.95, 7x7); configs[3] sharding at N>1",
                   "frames_per_gpu": B, "H": H, "W": W, "iters": ITERS, "parallelism": f"frame-parallel x{n_gpus}"},
    }
    if ws_ranks is not None:
        out["workspace_ranks"] = ws_ranks
    if dumped is not None:
        out["dumped_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    if args.stub_step:
        out["data"] = "stub step (rank-plumbing test, no GPU work)"
        if dist is not None:
            dist.destroy_process_group()
        print(json.dumps(out), flush=True)
        return

    # families = launches grouped by kernel name ("family:layer" -> "family")
    kern = {}
    for name, v in layers.items():
        fam = name.split(":", 1)[0]
        k = kern.setdefault(fam, {"calls": 0, "ms": 0.0, "flops": 0.0})
        k["calls"] += v["calls"]
        k["ms"] += v["ms"]
        k["flops"] += v.get("flops", 0.0)

    def per_launch(names):
        ms = sum(kern[n]["ms"] for n in names if n in kern)
        calls = sum(kern[n]["calls"] for n in names if n in kern)
        return ms, calls

    ks, tps, tr = {}, [], {}
    if kern:
        conv_names = ["igemm_conv", "igemm_conv_gru_zr", "igemm_conv_gru_q", "igemm_conv_flow"]
        ms, calls = per_launch(conv_names)
        steps = max(1, prof_steps)           # the steps whose launches carried events
        if ms > 0:
            executed = sum(kern[n]["flops"] for n in conv_names if n in kern)       # what the launches really multiplied
            if executed <= 0:
                executed = work["conv_flops_executed"] * steps
            tf_exec = executed / (ms * 1e-3) / 1e12
            tf_alg = work["conv_flops"] * steps / (ms * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "kernel": "igemm_kernel (fp32 MFMA implicit-GEMM conv, all epilogues)",
                               "achieved": round(tf_exec, 2), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(tf_exec / MFMA_F32_PEAK_TFLOPS, 4), "traffic": None,
                               "launches_per_step": calls // steps, "avg_launch_ms": round(ms / calls, 4), "profiled_steps": steps,
                               "flops_per_step_executed": executed / steps, "share_of_step": round(ms / steps / ms_per_step, 4),
                               "algorithmic_tflops": round(tf_alg, 2), "algorithmic_flops_per_step": work["conv_flops"],
                               "note": "achieved/frac = FLOPs the launches executed / HIP-event kernel time / fp32-MFMA peak; "
                                       "algorithmic_tflops prices the reference's convolution FLOPs (SURVEY 8d) instead: the GRU's "
                                       "loop-invariant context third is evaluated once per pair, an algorithmic saving, not "
                                       "hardware efficiency"}
        def hbm(name, key_bytes, label):
            m, c = per_launch([name])
            if c:
                per = work[key_bytes] / (c / steps)
                gbs = per / (m / c * 1e-3) / 1e9
                ks[label] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(gbs / HBM_PEAK_GBS, 4), "frac_of_achievable": round(gbs / HBM_ACHIEVABLE_GBS, 4),
                             "bytes_per_launch": per, "avg_launch_ms": round(m / c, 4), "launches_per_step": c // steps}
        vol_fam = "corr_vol_f32" if "corr_vol_f32" in kern else "igemm_corr_volume"    # the A-stationary kernel's fp32 form / the generic batched GEMM
        hbm(vol_fam, "volume_bytes", "corr_volume_gemm")
        hbm("corr_pyramid_pool", "pool_bytes", "corr_pyramid_pool")
        work["lookup_total"] = work["lookup_bytes"] * ITERS
        hbm("corr_lookup", "lookup_total", "corr_lookup")
        hbm("upsample_flow", "upsample_bytes", "upsample_flow")
        hbm("warp_u8", "warp_bytes", "warp")
        hbm("upsample_warp", "upsample_warp_bytes", "upsample_warp")
        hbm("generate_mask", "mask_bytes", "mask")
        m, c = per_launch([vol_fam])
        if c:
            ks["corr_volume_gemm"]["kernel"] = ("corr_vol_split_kernel<fp32> (A-stationary, v_mfma_f32_32x32x2_f32, LDS-DMA column stream, staged whole-line stores)"
                                                if vol_fam == "corr_vol_f32" else "igemm_kernel batched mode, epilogue kEpiVolPool")
            tfv = work["volume_flops"] * steps / (m * 1e-3) / 1e12
            ks["corr_volume_gemm"]["tflops"] = round(tfv, 2)
            ks["corr_volume_gemm"]["mfma_frac"] = round(tfv / MFMA_F32_PEAK_TFLOPS, 4)
        # HBM bytes per launch: PMC counters cannot be read from inside this process, so `traffic` is the figure of the
        # committed rocprofv3 --pmc passes of this same command (FETCH_SIZE / WRITE_SIZE in separate runs, corrected per
        # access width with the calibration kernels of tools/pmc_calibrate.py) and is labelled as such.
        import glob
        tps = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic_b64.json")))   # newest round last
        if B == 64 and tps:
            tp = tps[-1]
            tr = json.load(open(tp))
            src = f"profile: profiles/{os.path.basename(tp)} (committed rocprofv3 --pmc passes, not collected in this run)"
            # tie the profile to the binary being timed: the round tag / source revision it was taken at, and whether the
            # libofx.so it ran is byte for byte the one loaded here (a stale profile then says so itself)
            import hashlib
            meta = tr.pop("_profile", None) or {}
            try:
                here = hashlib.sha256(open(os.path.join(ROOT, "sd_animation_optical_flow_amd", "libofx.so"), "rb").read()).hexdigest()
            except OSError:
                here = None
            out["traffic_profile"] = {"file": f"profiles/{os.path.basename(tp)}", "tag": meta.get("tag"), "git_rev": meta.get("git_rev"),
                                      "libofx_sha256": meta.get("libofx_sha256"), "timed_libofx_sha256": here,
                                      "same_binary": bool(here) and here == meta.get("libofx_sha256")}
            if "roofline" in out and "igemm_conv_all" in tr:
                out["roofline"]["traffic"] = tr["igemm_conv_all"]["hbm_bytes_per_launch_corrected"]
                out["roofline"]["traffic_source"] = src
            for label, tkey in (("corr_volume_gemm", "corr_volume_gemm"), ("corr_lookup", "corr_lookup"),
                               ("corr_pyramid_pool", "pyramid_pool"), ("upsample_flow", "upsample"),
                               ("warp", "warp"), ("mask", "mask"), ("upsample_warp", "upsample_warp")):
                if label in ks and tkey in tr:
                    ks[label]["traffic"] = tr[tkey]["hbm_bytes_per_launch_corrected"]
                    ks[label]["traffic_source"] = "profile"
                    if ks[label].get("avg_launch_ms"):
                        gbs = ks[label]["traffic"] / (ks[label]["avg_launch_ms"] * 1e-3) / 1e9
                        ks[label]["traffic_gbs"] = round(gbs, 1)
                        ks[label]["traffic_frac"] = round(gbs / HBM_PEAK_GBS, 4)
        out["kernels"] = ks
        tot = sum(v["ms"] for v in kern.values())
        out["kernel_time_share"] = {k: round(v["ms"] / tot, 4) for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"])[:8]}
        # per-layer table of the convolutions (executed TFLOP/s per layer: the short-K layers are the visible deficit)
        rows = []
        for name, v in layers.items():
            if ":" in name and v.get("flops", 0) > 0 and name.split(":", 1)[0] in conv_names + ["igemm_corr_volume", "corr_vol_f32"]:
                rows.append({"layer": name.split(":", 1)[1], "calls_per_step": v["calls"] // steps,
                             "avg_ms": round(v["ms"] / v["calls"], 4), "ms_per_step": round(v["ms"] / steps, 3),
                             "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1)})
        rows.sort(key=lambda r: -r["ms_per_step"])
        out["layers"] = rows[:40]

    verify_path = None
    if not args.no_verify and last is not None:
        # three pairs of the LAST timed step, checked against the CPU oracle (fp32 and float64) outside the timed region
        import tempfile
        import numpy as np
        vb = sorted({0, B // 2, B - 1})
        flow, warped, mask = last
        fd, verify_path = tempfile.mkstemp(suffix=".npz", prefix="ofx_verify_")
        os.close(fd)
        pick = lambda t: t[vb].cpu().numpy()
        np.savez(verify_path, frame=pick(frames), key=key.cpu().numpy(), key_ai=key_ai.cpu().numpy(),
                 conf=pick(conf), flow=pick(flow), warped=pick(warped), mask=pick(mask), index=np.array(vb), warp_mode=args.warp_mode)
    del last

    if not args.no_single and world == 1:
        f1 = frames[:1].contiguous()
        c1 = conf[:1].contiguous()

        one_pair = make_step(eng, f1, key, key_ai, c1, args.warp_mode, args.separate_warp)
        for _ in range(2):
            one_pair()
        torch.cuda.synchronize()
        reps = 5
        t1 = time.perf_counter()
        for _ in range(reps):
            one_pair()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t1) / reps
        ops.prof_enable(1)                       # one more call, outside the timing, to count the FLOPs its launches execute
        one_pair()
        fam = ops.prof_collect()
        ops.prof_enable(False)
        out["single_pair"] = {"workload": "BASELINE configs[1]: one 512x768 pair", "ms": round(dt * 1e3, 3), "pairs_per_s": round(1 / dt, 2)}
        # roofline of the single pair: every launch here is a grid of 100-400 workgroups on 256 CUs, so this is a latency / fill
        # figure -- executed convolution FLOPs of the whole call over its WALL time against the fp32 MFMA peak (the convolutions are
        # spread over three streams: summing their event times would count overlapped work twice)
        cf = sum(v.get("flops", 0.0) for k, v in fam.items() if k.startswith("igemm_conv"))
        if cf > 0:
            tf1 = cf / dt / 1e12
            out["single_pair"]["roofline"] = {"bound": "mfma", "achieved": round(tf1, 2), "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s",
                                              "frac": round(tf1 / MFMA_F32_PEAK_TFLOPS, 4), "flops_executed": cf,
                                              "note": "executed convolution FLOPs / wall time of the whole call (flow + warp + mask)"}

    if not args.no_sweep and not args.no_single and world == 1 and B >= 16:
        # the batches between configs[1] and configs[2]: what a frame-by-frame caller (B = 1, the reference's README path), a
        # forward-backward `calc` (2), `PDCNetAux`'s batches (16, ofgen_keyframe_inpaint.py:1128) and short segments see
        sweep = [{"B": 1, "ms": out["single_pair"]["ms"], "pairs_per_s": out["single_pair"]["pairs_per_s"]}]
        for bs in (4, 16):
            sstep = make_step(eng, frames[:bs].contiguous(), key, key_ai, conf[:bs].contiguous(), args.warp_mode, args.separate_warp)
            for _ in range(2):
                sstep()
            torch.cuda.synchronize()
            reps = 5 if bs <= 4 else 3
            t1 = time.perf_counter()
            for _ in range(reps):
                sstep()
            torch.cuda.synchronize()
            dts = (time.perf_counter() - t1) / reps
            sweep.append({"B": bs, "ms": round(dts * 1e3, 3), "pairs_per_s": round(bs / dts, 2)})
            del sstep
        sweep.append({"B": B, "ms": round(ms_per_step, 3), "pairs_per_s": round(B / ms_per_step * 1e3, 2)})
        out["batch_sweep"] = sweep

    if not args.no_fast and world == 1 and args.precision == "fp32":
        # `ofgen.RAFT_2` AS WRITTEN (the reference never calls .eval(): context-encoder BatchNorm on each image's own statistics,
        # ofgen_keyframe_inpaint.py:47-60) on the same clip and the same step: a second copy of the context encoder without folded
        # statistics + per-image statistics and their apply passes.  Secondary line; `value` stays on the eval-mode network.
        engb = RaftEngine(random_state_dict(0), dev, precision="fp32", cnet_norm="batch")
        bstep = make_step(engb, frames, key, key_ai, conf, args.warp_mode, args.separate_warp)
        fb = bstep()[0]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            bstep()
        torch.cuda.synchronize()
        dtb = (time.perf_counter() - t1) / args.steps
        out["raft2_as_written"] = {"cnet_norm": "batch", "value": round(B / dtb, 3), "unit": "pairs/s", "ms_per_step": round(dtb * 1e3, 3),
                                   "note": "the reference's RAFT_2 as written (BatchNorm on per-image statistics); same step, same clip"}
        if verify_path:
            import numpy as np
            z = dict(np.load(verify_path))
            z["flow_bn_batch"] = fb[:1].cpu().numpy()
            np.savez(verify_path, **z)
        del engb, bstep, fb

    if not args.no_handoff and world == 1:
        # BASELINE configs[4]'s frame size, the half of it that is on the path: warp/mask outputs -> Pillow-exact inpaint inputs ->
        # first-stage latent, one 1024x1024 frame per call, everything resident in HBM
        from sd_animation_optical_flow_amd import handoff
        from sd_animation_optical_flow_amd.vae import VaeEncoder, random_vae_state_dict
        g5 = torch.Generator(device=dev).manual_seed(5)
        fr5 = torch.randint(0, 256, (1, 1024, 1024, 3), dtype=torch.uint8, device=dev, generator=g5)
        rf5 = torch.randint(0, 256, (1, 1024, 1024, 3), dtype=torch.uint8, device=dev, generator=g5)
        mk5 = (torch.rand((1, 1024, 1024), device=dev, generator=g5) > 0.8).to(torch.uint8) * 255
        vae = VaeEncoder(random_vae_state_dict(0), dev)

        def hstep():
            t5 = handoff.prepare_inpaint_inputs(fr5, rf5, mk5, mask_blur=4, device=dev)
            return vae.get_first_stage_encoding(t5["image"])
        for _ in range(2):
            hstep()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(5):
            z5 = hstep()
        torch.cuda.synchronize()
        out["sd_handoff_1024"] = {"workload": "BASELINE configs[4] frame size, non-generative half: inpaint inputs + first-stage latent, one 1024x1024 frame",
                                  "ms": round((time.perf_counter() - t1) / 5 * 1e3, 3), "finite": bool(torch.isfinite(z5).all())}
        del vae, fr5, rf5, mk5

    if not args.no_volsplit and world == 1 and args.precision == "fp32":
        # ONLY the all-pairs correlation volume (RAFT/core/corr.py:52-60) on the bf16 matrix cores, operands pre-split into bf16 planes
        # (csrc/corr_split.hip; RaftEngine(volume_precision=...)); every convolution stays exact fp32.  Secondary lines: `value` above is
        # the pure-fp32 step.  Kernel time from HIP events of one extra step; the flows of the verified pairs join the oracle check.
        ref_flow = eng.forward(frames, key, iters=ITERS)
        vs = {}
        for mode, fam, nprod in (("bf16x6", "corr_vol_split6", 6), ("bf16x3", "corr_vol_split3", 3)):
            engv = RaftEngine(random_state_dict(0), dev, precision="fp32", volume_precision=mode)
            vstep = make_step(engv, frames, key, key_ai, conf, args.warp_mode, args.separate_warp)
            fl = vstep()[0]
            epe = float((fl - ref_flow).pow(2).sum(-1).sqrt().mean())
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                vstep()
            torch.cuda.synchronize()
            dtv = (time.perf_counter() - t1) / args.steps
            ops.prof_enable(1)
            for _ in range(3):                 # three launches: a single one is at the mercy of the clock it happens to get
                vstep()
            fk = ops.prof_collect()
            ops.prof_enable(False)
            gm = fk.get(fam, {}).get("ms")
            sp = fk.get("corr_split_planes", {}).get("ms")
            gm = gm / 3 if gm else gm
            sp = sp / 3 if sp else sp
            rec = {"precision": mode, "products_per_fp32_product": nprod, "kernel": "corr_vol_split_kernel (A-stationary, LDS-DMA column stream, staged whole-line stores)",
                   "step_value": round(B / dtv, 3), "step_unit": "pairs/s", "step_ms": round(dtv * 1e3, 3), "flow_epe_vs_fp32_engine_px": epe}
            if gm:
                gbs = work["volume_bytes"] / (gm * 1e-3) / 1e9
                tfx = work["volume_flops"] * nprod / (gm * 1e-3) / 1e12
                rec.update({"bound": "hbm", "avg_launch_ms": round(gm, 4), "split_planes_ms": round(sp, 4) if sp else None,
                            "bytes_per_launch": work["volume_bytes"], "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(gbs / HBM_PEAK_GBS, 4), "frac_of_achievable": round(gbs / HBM_ACHIEVABLE_GBS, 4),
                            "bf16_mfma_tflops_executed": round(tfx, 1), "bf16_mfma_frac": round(tfx / MFMA_BF16_PEAK_TFLOPS, 4),
                            "fp32_gemm_ms": ks.get("corr_volume_gemm", {}).get("avg_launch_ms")})
                tkey = "corr_vol_split6" if nprod == 6 else "corr_vol_split3"
                if B == 64 and tps and tkey in tr:
                    rec["traffic"] = tr[tkey]["hbm_bytes_per_launch_corrected"]
                    rec["traffic_ratio"] = round(rec["traffic"] / work["volume_bytes"], 3)
                    rec["traffic_source"] = "profile"
            vs[mode] = rec
            if verify_path:
                import numpy as np
                z = dict(np.load(verify_path))
                z["flow_vol_" + mode] = fl[sorted({0, B // 2, B - 1})].cpu().numpy()
                np.savez(verify_path, **z)
            del engv, vstep, fl
        del ref_flow
        out.setdefault("kernels", {})["corr_volume_gemm_split"] = vs

    if not args.no_fast and world == 1 and args.precision == "fp32":
        # secondary measurement: the opt-in split-bf16 mode on the same clip, with its flow error against the fp32 run
        ref_flow = eng.forward(frames, key, iters=ITERS)
        for mode, key_name, note in (("bf16x3", "fast_mode", "opt-in; not the headline value (the reference computes in fp32)"),
                                     ("bf16x6", "split3_mode", "opt-in; three bf16 pieces per fp32 operand (exact), six products, fp32 accumulate: "
                                      "fp32-level accuracy on the bf16 matrix cores; not the headline value")):
            fast = RaftEngine(random_state_dict(0), dev, precision=mode)
            # the SAME step as `value` (make_step: the product's FrameSynthesizer, warp inside the convex upsample), with the engine
            # built in that mode -- what test_split_modes_at_the_bench_size_against_the_oracles holds to the oracles
            mstep = make_step(fast, frames, key, key_ai, conf, args.warp_mode, args.separate_warp)

            def fstep():
                return mstep()[0]
            fl = fstep()
            epe = float((fl - ref_flow).pow(2).sum(-1).sqrt().mean())
            emax = float((fl - ref_flow).pow(2).sum(-1).sqrt().max())
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(args.steps):
                fstep()
            torch.cuda.synchronize()
            dtf = (time.perf_counter() - t1) / args.steps
            out[key_name] = {"precision": mode, "value": round(B / dtf, 3), "unit": "pairs/s", "ms_per_step": round(dtf * 1e3, 3),
                             "flow_epe_vs_fp32_px": epe, "flow_max_err_vs_fp32_px": emax, "note": note}
            del fast, mstep
        del ref_flow

    if not args.no_pipeline and world == 1 and args.precision == "fp32":
        # the path end to end over a workspace (SURVEY 8e names a rank's host side as the scaling limit): PNGs on disk -> decode ->
        # H2D -> flow both ways + confidence -> warp + mask -> SD-inpaint inputs -> render -> D2H -> PNGs on disk, against the same
        # calls on resident frames.  Needs a writable temp dir; never `value` (inputs of `value` are resident in HBM).
        import tempfile
        try:
            with tempfile.TemporaryDirectory(prefix="ofx_probe_"):
                pass
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import pipeline_rate
            wp = pipeline_rate.measure(128, None, reps=1, inline=False)
            wp["one_batch_share"] = {k: v for k, v in pipeline_rate.measure(64, None, reps=1, inline=False).items()
                                     if k in ("frames", "end_to_end_fps", "device_only_fps", "ratio", "host_cpu_s_per_frame", "edge_batch")}
            out["workspace_pipeline"] = wp
        except Exception as e:                                   # read-only or missing temp dir, Pillow absent ...: report, do not fail the bench
            out["workspace_pipeline"] = {"error": repr(e)[:200]}

    # child process with a hard time limit: neither the baseline nor the check may take the GPU number down with them
    import subprocess
    want_base = not args.no_cpu_baseline and world == 1
    if want_base or verify_path:
        cmd = [sys.executable, os.path.abspath(__file__)]
        cmd += ["--cpu-baseline-only"] if want_base else ["--verify-only"]
        if verify_path:
            cmd += ["--verify-npz", verify_path]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
            res = json.loads(r.stdout.strip().splitlines()[-1])
            ver = res.pop("verified", None)
            if want_base:
                out["cpu_baseline"] = res
            if ver is not None:
                out["verified"] = ver
                out["verified_epe"] = ver["flow_epe_px"]
        except Exception as e:
            if want_base:
                out["cpu_baseline"] = {"value": None, "unit": "pairs/s", "cores": usable_cores(), "kind": "port", "error": repr(e)[:200]}
            if verify_path:
                out["verified"] = {"error": repr(e)[:200]}
        finally:
            if verify_path and os.path.exists(verify_path):
                os.unlink(verify_path)
    if dist is not None:
        dist.destroy_process_group()       # before the result line: RCCL prints its own banner lines on teardown
    flush_c_stdio()
    sys.stderr.flush()
    print(json.dumps(out), flush=True)      # the ONE JSON line, last thing on stdout


if __name__ == "__main__":
    main()
