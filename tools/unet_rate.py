#!/usr/bin/env python3
"""`UNetModel` rate on the full SD v1.5 configuration: the default path (ofx_groupnorm_cat reading the two halves of every
concatenation and folding the emb term, ofx_emb_linear, ofx_timestep_embedding) against the composition that was possible before
them (OFX_UNET_TORCH_GLUE=1: torch.cat + ofx_groupnorm, the emb term as a torch broadcast add, the timestep path through
torch.nn.functional), on the same commit and the same library.

Workload: `SD_V15_UNET` (in_channels 9) with seeded weights, batch 2 (cond / uncond), a 64 x 96 latent (a 512 x 768 frame), 77 x 768
context, no control, no reference K/V.

OFX_UNET_TORCH_GLUE is read once per process, so each variant runs in a child process of its own; the children alternate for
`--rounds` rounds so that drift and other tenants hit both.  A figure is device-event time per forward over `--reps` back-to-back
calls of `forward_nhwc` after `--warmup` calls; each line gives the mean over rounds with the fastest and slowest round behind it.

kernels: in the last round, after the timed window, the library's event profiler (ofx_prof_enable) brackets every launch of the
library for `--reps` more forwards: ms per forward and launches per forward by kernel kind.  torch's own kernels (the glue variant's
cat / add / linear, the control additions) are not in that table; their time is in the ms per forward.  The event pairs serialise
the launches, so the table's sum exceeds the timed figure's share.

--precision A,B,...: compare `UNetModel(precision=)` values instead (each of "fp32", "fp16", "bf16x3", "bf16x6"; the default path, no
glue), in alternating fresh processes, rounds and statistics as above; the first one named is the baseline of the ratios, and every
variant gets its launch table.  The fp32 row is measured in the same session as the others, never copied.

--attention-precision A,B: with it every --precision is run with each `UNetModel(attention_precision=)` named ("fp32", "fp16"), e.g.
--precision fp32,fp16 --attention-precision fp32,fp16 is the four-way comparison fp32+attn-fp32 (the baseline), fp32+attn-fp16,
fp16+attn-fp32, fp16+attn-fp16.

--sincos-probe PATH: also run the cosf / sinf probe (tools/sincos_probe.hip, built beforehand) over the arguments of the
timestep-embedding test grid (tests/unet_check.sincos_arguments) and report the device's worst error against float64 in units of
2^-24: Y_SINCOS.

    python tools/unet_rate.py [--out profiles/r20_unet_rate.txt] [--sincos-probe ./sincos_probe]
    python tools/unet_rate.py --precision fp32,bf16x3,fp16 [--out profiles/r23_unet_f16_rate.txt]
    python tools/unet_rate.py --precision fp32,fp16 --attention-precision fp32,fp16
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH, LAT_H, LAT_W, CTX_TOKENS = 2, 64, 96, 77
KINDS = (("convolutions and the transformers' GEMMs", ("igemm_conv",)), ("upconv2x", ("upconv2x",)),
         ("attention", ("attn_flash", "attn_flash_bnhd", "attn_flash_f16", "attn_flash_bnhd_f16", "softmax_rows", "attn_pack", "attn_nan_rows")),
         ("groupnorm_cat partial sums", ("groupnorm_cat_partial",)), ("groupnorm_cat finalize", ("groupnorm_cat_finalize",)),
         ("groupnorm_cat apply", ("groupnorm_cat_apply",)), ("groupnorm (ofx_groupnorm)", ("groupnorm_stats", "groupnorm_apply")),
         ("emb_linear", ("emb_linear",)), ("timestep_embedding", ("timestep_embedding",)), ("layernorm", ("layernorm",)),
         ("geglu", ("geglu",)))


def child(reps: int, warmup: int, profile: bool, precision: str, attention_precision: str = "fp32") -> None:
    import torch
    from sd_animation_optical_flow_amd import ops
    from sd_animation_optical_flow_amd import unet as UN
    assert torch.cuda.is_available(), "a GPU is needed: nothing here is measured on the host"
    cfg = UN.SD_V15_UNET
    model = UN.UNetModel(UN.random_unet_state_dict(0, cfg), cfg, prefix="", precision=precision, attention_precision=attention_precision)
    assert set(model.attention_precision_of.values()) == {attention_precision}       # all 16 transformers of SD v1.5 take it
    g = torch.Generator().manual_seed(20)
    x = torch.randn((BATCH, LAT_H, LAT_W, cfg["in_channels"]), generator=g).cuda()
    t = torch.tensor([981.0, 981.0]).cuda()
    ctx = torch.randn((BATCH, CTX_TOKENS, cfg["context_dim"]), generator=g).cuda()
    out, hist = model.forward_nhwc(x, t, ctx)
    res = {"glue": UN._torch_glue(), "precision": model.precision, "attention_precision": model.attention_precision, "checksum": float(out.double().abs().mean()), "transformers": len(hist)}
    for _ in range(warmup):
        model.forward_nhwc(x, t, ctx)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        model.forward_nhwc(x, t, ctx)
    e1.record()
    torch.cuda.synchronize()
    res["ms"] = e0.elapsed_time(e1) / reps
    if profile:
        ops.prof_enable(1)
        ops.prof_collect()
        for _ in range(reps):
            model.forward_nhwc(x, t, ctx)
        res["kernels"] = ops.prof_collect()
        ops.prof_enable(0)
    print("RESULT " + json.dumps(res))


def measure_sincos(probe: str) -> str:
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import unet_check as UC
    a = UC.sincos_arguments()
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.f32")
        a.numpy().tofile(fin)
        subprocess.run([probe, fin, fout], check=True, timeout=120)
        dev = torch.from_numpy(np.fromfile(fout, dtype=np.float32)).view(2, -1)
    ref = torch.stack([torch.cos(a.double()), torch.sin(a.double())])
    err = (dev.double() - ref).abs() / UC.U
    host = (torch.stack([torch.cos(a), torch.sin(a)]).double() - ref).abs() / UC.U
    ic, is_ = int(err[0].argmax()), int(err[1].argmax())
    return (f"cosf / sinf on the device over {a.numel()} arguments of the timestep-embedding test grid (t in {UC.TS_T} times the "
            f"frequency tables of dims {UC.TS_DIMS}, and a sweep of 0..1000 rad):\n"
            f"  worst |cosf(a) - cos64(a)| = {float(err[0].max()):.3f} u at a = {float(a[ic]):.6g}, "
            f"worst |sinf(a) - sin64(a)| = {float(err[1].max()):.3f} u at a = {float(a[is_]):.6g}   (u = 2^-24, absolute; torch's "
            f"float32 cos / sin on the host over the same arguments: {float(host[0].max()):.3f} / {float(host[1].max()):.3f})\n")


def kernel_table(label: str, k: dict, reps: int) -> list:
    lines = [f"{label}: the library's launches per forward, event profiler over {reps} forwards"]
    tot_ms, tot_n = 0.0, 0.0
    rows = [(lab, names) for lab, names in KINDS]
    rows.append(("the rest", tuple(n for n in k if not any(n in names for _, names in KINDS))))
    for lab, names in rows:
        ms = sum(k[n]["ms"] for n in names if n in k) / reps
        n = sum(k[n]["calls"] for n in names if n in k) / reps
        tot_ms, tot_n = tot_ms + ms, tot_n + n
        if n:
            lines.append(f"  {lab:44s} {ms:9.3f} ms  {n:7.1f} launches  {1e3 * ms / n:8.1f} us each")
    lines.append(f"  {'all':44s} {tot_ms:9.3f} ms  {tot_n:7.1f} launches")
    lines.append("")
    return lines


def run_child(a, rnd: int, env: dict, precision: str, attention_precision: str = "fp32") -> dict:
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup), "--child-precision", precision,
           "--child-attention-precision", attention_precision]
    if rnd == a.rounds - 1:
        cmd.append("--profile")
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
    if r.returncode != 0:
        sys.exit(f"child failed ({r.returncode}); nothing further is started\n{r.stdout}\n{r.stderr}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def compare_precisions(a) -> str:
    precs = [p.strip() for p in (a.precision or "fp32").split(",") if p.strip()]
    if a.attention_precision:                                       # every precision with every attention precision, e.g. "fp16+attn-fp16"
        aps = [p.strip() for p in a.attention_precision.split(",") if p.strip()]
        variants = {f"{p}+attn-{q}": (p, q) for p in precs for q in aps}
    else:
        variants = {p: (p, "fp32") for p in precs}
    precs = list(variants)
    runs = {p: [] for p in precs}
    for rnd in range(a.rounds):
        for p in precs:
            res = run_child(a, rnd, dict(os.environ, OFX_UNET_TORCH_GLUE="0"), *variants[p])
            assert (res["precision"], res["attention_precision"]) == variants[p] and not res["glue"]
            runs[p].append(res)
            print(f"round {rnd} {p}: {res['ms']:.3f} ms", flush=True)
    stat = lambda v: f"{sum(v) / len(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
    ms = {p: [r["ms"] for r in runs[p]] for p in precs}
    mean = {p: sum(v) / len(v) for p, v in ms.items()}
    base = precs[0]
    lines = [f"UNetModel.forward_nhwc(precision=), SD v1.5 configuration (in_channels 9, {runs[base][0]['transformers']} transformers), seeded "
             f"weights, batch {BATCH}, latent {LAT_H} x {LAT_W}, context {CTX_TOKENS} x 768; ms per forward, device events over {a.reps} forwards, "
             f"mean of {a.rounds} rounds [fastest .. slowest], the precisions in alternating fresh processes of one session", ""]
    for p in precs:
        lines.append(f"  {p:15s} {stat(ms[p])} ms   mean |out| {runs[p][0]['checksum']:.6f}")
    lines.append("")
    for p in precs[1:]:
        clear = max(ms[p]) < min(ms[base]) or min(ms[p]) > max(ms[base])
        lines.append(f"  {base} / {p} = {mean[base] / mean[p]:.3f}   ({'the brackets do not overlap' if clear else 'THE BRACKETS OVERLAP: inside the run-to-run spread'})")
    for i, p in enumerate(precs[1:], 1):
        for q in precs[i + 1:]:
            lines.append(f"  {p} / {q} = {mean[p] / mean[q]:.3f}")
    lines.append("")
    for p in precs:
        lines += kernel_table(p, runs[p][-1].get("kernels", {}), a.reps)
    return "\n".join(lines)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--sincos-probe")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--precision", help="comma-separated UNetModel precisions to compare, the baseline first (e.g. fp32,bf16x3,fp16)")
    ap.add_argument("--attention-precision", help="comma-separated UNetModel attention_precision values (fp32,fp16): every --precision is "
                                                  "run with each of them, the variants named e.g. fp16+attn-fp16")
    ap.add_argument("--child-precision", default="fp32")
    ap.add_argument("--child-attention-precision", default="fp32")
    a = ap.parse_args()
    if a.child:
        child(a.reps, a.warmup, a.profile, a.child_precision, a.child_attention_precision)
        return
    if a.precision or a.attention_precision:
        text = compare_precisions(a)
        print(text)
        if a.out:
            with open(a.out, "w") as f:
                f.write(text + "\n")
        return
    runs = {False: [], True: []}
    for rnd in range(a.rounds):
        for glue in (False, True):
            res = run_child(a, rnd, dict(os.environ, OFX_UNET_TORCH_GLUE="1" if glue else "0"), "fp32")
            assert res["glue"] == glue
            runs[glue].append(res)
            print(f"round {rnd} {'glue' if glue else 'default'}: {res['ms']:.3f} ms", flush=True)
    stat = lambda v: f"{sum(v) / len(v):8.3f} [{min(v):7.3f} .. {max(v):7.3f}]"
    dv, gv = [r["ms"] for r in runs[False]], [r["ms"] for r in runs[True]]
    lines = [f"UNetModel.forward_nhwc, SD v1.5 configuration (in_channels 9, {runs[False][0]['transformers']} transformers), seeded weights, "
             f"batch {BATCH}, latent {LAT_H} x {LAT_W}, context {CTX_TOKENS} x 768; ms per forward, device events over {a.reps} forwards, "
             f"mean of {a.rounds} rounds [fastest .. slowest], default and glue in alternating fresh processes",
             "default = ofx_groupnorm_cat (two pointers, emb term folded) + ofx_emb_linear + ofx_timestep_embedding; glue = "
             "OFX_UNET_TORCH_GLUE=1 (torch.cat + ofx_groupnorm, torch broadcast add, torch.nn.functional timestep path)", "",
             f"  default {stat(dv)} ms", f"  glue    {stat(gv)} ms", f"  glue / default = {sum(gv) / sum(dv):.3f}",
             f"  mean |out|: default {runs[False][0]['checksum']:.6f}, glue {runs[True][0]['checksum']:.6f}", ""]
    for glue in (False, True):
        lines += kernel_table("glue" if glue else "default", runs[glue][-1].get("kernels", {}), a.reps)
    if a.sincos_probe:
        lines.append(measure_sincos(a.sincos_probe))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
