#!/usr/bin/env python3
"""`SpatialTransformer` rate at the SD-v1 level shapes of a 512x768 frame: the default path (ofx_layernorm, ofx_geglu, attention on
token rows) against the PyTorch glue it replaces (OFX_ST_TORCH_GLUE=1), and the new kernels on their own.

Batch 2 (cond / uncond), 77 x 768 context, seeded weights, one transformer block per level:
    6144 tokens x 320 channels, 8 heads of 40      (64 x 96 latent)
    1536 tokens x 640 channels, 8 heads of 80
     384 tokens x 1280 channels, 8 heads of 160
each with and without one reference frame's K/V (batch 2: every image attends to the reference's keys alone).

OFX_ST_TORCH_GLUE is read once per process, so each variant runs in a child process of its own; the children alternate for
`--rounds` rounds so that drift and other tenants hit both.  A figure is device-event time per call over `--reps` back-to-back
calls after a warm-up at the same shape; each line gives the mean over rounds with the fastest and slowest round behind it.

kernels: in the default child, after the timed windows, the library's event profiler (ofx_prof_enable) brackets every launch of
`--reps` more calls; "layernorm", "geglu" and "attn_flash_bnhd" are reported per launch.  For the two bandwidth-bound kernels the
algorithmic bytes (LayerNorm: the row read and written once; GEGLU: two inputs read, one output written) over that time are given
as a fraction of the 8 TB/s HBM specification, the figure the README uses.  The attention kernel is given in TFLOP/s
(4 B H Nq Nk D).

--erff-probe PATH: also run the erff probe (tools/erff_probe.hip, built beforehand) over the arguments of the GEGLU test grid
(tests/transformer_check.py) and report the worst error of the device's erff against float64 erf in units of 2^-24 |erf|: Y_ERF.

    python tools/spatial_transformer_rate.py [--out profiles/r17_spatial_transformer_rate.txt] [--erff-probe ./erff_probe]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = [(320, 8, 40, 64, 96), (640, 8, 80, 32, 48), (1280, 8, 160, 16, 24)]      # channels, heads, d_head, h, w
BATCH, CTX_TOKENS, CTX_DIM = 2, 77, 768
HBM_SPEC = 8.0e12


def child(reps: int, warmup: int, profile: bool) -> None:
    import torch
    from sd_animation_optical_flow_amd import ops
    from sd_animation_optical_flow_amd import transformer as T
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    res = {"glue": T._torch_glue(), "levels": []}
    for Cn, heads, d, h, w in LEVELS:
        mod = T.SpatialTransformer(T.random_spatial_transformer_state_dict(0, Cn, heads, d, CTX_DIM), heads, d)
        g = torch.Generator().manual_seed(Cn)
        x = torch.randn((BATCH, h, w, Cn), generator=g).cuda()
        ctx = torch.randn((BATCH, CTX_TOKENS, CTX_DIM), generator=g).cuda()
        out0, hist = mod.forward_nhwc(x, ctx)
        ref = [hist[0]]                                              # one reference frame's K/V, batch B
        row = {"C": Cn, "tokens": h * w, "checksum": float(out0.double().abs().mean())}
        for name, kw in (("plain", {}), ("ref_kv", {"reference_kv": ref})):
            for _ in range(warmup):
                mod.forward_nhwc(x, ctx, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                mod.forward_nhwc(x, ctx, **kw)
            e1.record()
            torch.cuda.synchronize()
            row[name + "_ms"] = e0.elapsed_time(e1) / reps
        if profile:
            ops.prof_enable(1)
            ops.prof_collect()
            for _ in range(reps):
                mod.forward_nhwc(x, ctx)
            prof = ops.prof_collect()
            ops.prof_enable(0)
            row["kernels"] = {k: prof[k] for k in ("layernorm", "geglu", "attn_flash_bnhd") if k in prof}
        res["levels"].append(row)
        del mod
    print("RESULT " + json.dumps(res))


def measure_erff(probe: str) -> str:
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import transformer_check as TC
    gen = torch.Generator().manual_seed(5)
    gates = torch.cat([TC.geglu_gates(1 << 20, gen), torch.linspace(-8.0, 8.0, 1 << 20)])
    t = TC.erff_arguments(gates).contiguous()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.f32")
        t.numpy().tofile(fin)
        subprocess.run([probe, fin, fout], check=True, timeout=120)
        import numpy as np
        dev = torch.from_numpy(np.fromfile(fout, dtype=np.float32))
    ref = torch.erf(t.double())
    ok = ref != 0
    err = (dev.double() - ref).abs()[ok] / (TC.U * ref.abs()[ok])
    i = int(err.argmax())
    host = ((torch.erf(t).double() - ref).abs()[ok] / (TC.U * ref.abs()[ok])).max()
    sat = bool((dev[t <= -6.0] == -1.0).all()) and bool((dev[t >= 6.0] == 1.0).all())
    return (f"erff on the device over {t.numel()} arguments of the GEGLU test grid (gates of tests/transformer_check.geglu_gates and a "
            f"sweep of -8..8, times fl(2^-1/2)):\n  worst |erff(t) - erf64(t)| = {float(err.max()):.3f} u |erf t| at t = {float(t[ok][i]):.6g}"
            f"   (u = 2^-24; torch's float32 erf on the host over the same arguments: {float(host):.3f})\n"
            f"  zero arguments give {sorted(set(dev[t == 0].tolist()))}; |t| >= 6 gives exactly +-1: {sat}\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--erff-probe")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.reps, a.warmup, a.profile)
        return
    runs = {False: [], True: []}
    for rnd in range(a.rounds):
        for glue in (False, True):
            env = dict(os.environ, OFX_ST_TORCH_GLUE="1" if glue else "0")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)]
            if not glue and rnd == a.rounds - 1:
                cmd.append("--profile")
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"child failed ({r.returncode}); nothing further is started\n{r.stdout}\n{r.stderr}")
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            assert res["glue"] == glue
            runs[glue].append(res)
    lines = [f"SpatialTransformer.forward_nhwc, batch {BATCH}, context {CTX_TOKENS} x {CTX_DIM}, depth 1; ms per call, device events over "
             f"{a.reps} calls, mean of {a.rounds} rounds [fastest .. slowest]; default = HIP LayerNorm / GEGLU / attention on token rows, "
             f"glue = OFX_ST_TORCH_GLUE=1 (torch LayerNorm / GEGLU, permute + ops.attention)", ""]
    stat = lambda v: f"{sum(v) / len(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
    for li, (Cn, heads, d, h, w) in enumerate(LEVELS):
        lines.append(f"{h * w} tokens x {Cn} channels, {heads} heads of {d}:")
        for name in ("plain", "ref_kv"):
            dv = [r["levels"][li][name + "_ms"] for r in runs[False]]
            gv = [r["levels"][li][name + "_ms"] for r in runs[True]]
            lines.append(f"  {name:7s} default {stat(dv)}   glue {stat(gv)}   glue / default = {sum(gv) / sum(dv):.3f}")
        c0, c1 = runs[False][0]["levels"][li]["checksum"], runs[True][0]["levels"][li]["checksum"]
        lines.append(f"  mean |out|: default {c0:.6f}, glue {c1:.6f}")
        k = runs[False][-1]["levels"][li].get("kernels", {})
        rows, inner = BATCH * h * w, Cn
        for nm, nbytes in (("layernorm", 2.0 * rows * inner * 4), ("geglu", 3.0 * rows * 4 * inner * 4)):
            if nm in k and k[nm]["calls"]:
                us = 1e3 * k[nm]["ms"] / k[nm]["calls"]
                lines.append(f"  {nm:16s} {us:8.1f} us per launch ({k[nm]['calls']} launches), {nbytes / 1e6:7.2f} MB -> "
                             f"{nbytes / (us * 1e-6) / 1e12:.2f} TB/s = {nbytes / (us * 1e-6) / HBM_SPEC:.2f} of the 8 TB/s HBM specification")
        if "attn_flash_bnhd" in k and k["attn_flash_bnhd"]["calls"]:
            kk = k["attn_flash_bnhd"]
            lines.append(f"  {'attn_flash_bnhd':16s} {1e3 * kk['ms'] / kk['calls']:8.1f} us per launch ({kk['calls']} launches: self- and "
                         f"cross-attention), {kk['flops'] / (kk['ms'] * 1e-3) / 1e12:.1f} TFLOP/s over both")
        lines.append("")
    if a.erff_probe:
        lines.append(measure_erff(a.erff_probe))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
