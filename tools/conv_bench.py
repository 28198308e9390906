#!/usr/bin/env python3
"""Micro-benchmark of the implicit-GEMM kernel on the update-block / encoder shapes (B=64 @512x768).
usage: python tools/conv_bench.py [libofx variant .so ...]
CONV_BENCH_WINO4=1: the Winograd F(4x4,3x3) kernel against F(2x2,3x3) over the batch sizes that set its gate;
CONV_BENCH_WINO4_ENC=1: the same on the encoders' stages, fused norm, statistics and residual merge included."""
import ctypes as C, sys, os, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sd_animation_optical_flow_amd import _lib
SHAPES = [  # name, B, H, W, Cin, Cout, kh, kw, stride, tile
    ("gru 1x5 256->256", 64, 96, 64, 256, 256, 1, 5, 1, 0),
    ("gru 5x1 256->128", 64, 96, 64, 256, 128, 5, 1, 1, 0),
    ("3x3 256->192", 64, 96, 64, 256, 192, 3, 3, 1, 0),
    ("3x3 128->256", 64, 96, 64, 128, 256, 3, 3, 1, 0),
    ("1x1 324->256", 64, 96, 64, 324, 256, 1, 1, 1, 0),
    ("enc 3x3 64->64 @1/2", 16, 384, 256, 64, 64, 3, 3, 1, 0),
    ("enc 3x3 96->96 @1/4", 16, 192, 128, 96, 96, 3, 3, 1, 0),
]
TILES = [0, 128128, 16128128, 128064, 16128064, 64064, 16064064]
if os.environ.get("CONV_BENCH_N64"):
    SHAPES = [
        ("enc 3x3 64->64 @1/2", 64, 384, 256, 64, 64, 3, 3, 1, 0),
        ("enc 7x7 4->64 s2", 64, 768, 512, 4, 64, 7, 7, 2, 0),
        ("3x3 128->64", 64, 96, 64, 128, 64, 3, 3, 1, 0),
        ("3x3 256->64", 64, 96, 64, 256, 64, 3, 3, 1, 0),
        ("3x3 512->64", 64, 96, 64, 512, 64, 3, 3, 1, 0),
        ("3x3 64->64 @1/8", 64, 96, 64, 64, 64, 3, 3, 1, 0),
        ("1x1 64->64 @1/2", 64, 384, 256, 64, 64, 1, 1, 1, 0),
    ]
    TILES = [0, 16128064, 16256064]
if os.environ.get("CONV_BENCH_B1"):
    SHAPES = [
        ("b1 gru 1x5 256->256", 1, 96, 64, 256, 256, 1, 5, 1, 0),
        ("b1 gru 5x1 256->128", 1, 96, 64, 256, 128, 5, 1, 1, 0),
        ("b1 3x3 256->192", 1, 96, 64, 256, 192, 3, 3, 1, 0),
        ("b1 3x3 128->256", 1, 96, 64, 128, 256, 3, 3, 1, 0),
        ("b1 1x1 324->256", 1, 96, 64, 324, 256, 1, 1, 1, 0),
        ("b1 enc 3x3 64->64 @1/2", 1, 384, 256, 64, 64, 3, 3, 1, 0),
        ("b1 enc 3x3 128->128 @1/8", 1, 96, 64, 128, 128, 3, 3, 1, 0),
    ]


if os.environ.get("CONV_BENCH_96"):      # the encoders' 96-channel stage at the bench batch (quarter resolution)
    SHAPES = [
        ("warm-up 3x3 256->192", 64, 96, 64, 256, 192, 3, 3, 1, 0),
        ("enc 3x3 96->96 @1/4 B64", 64, 192, 128, 96, 96, 3, 3, 1, 0),
    ]
    TILES = [0, 16256096]
if os.environ.get("CONV_BENCH_C1"):      # the motion encoder's 1x1 over the correlation channels, as laid out today and padded to whole chunks
    SHAPES = [
        ("warm-up 3x3 256->192", 64, 96, 64, 256, 192, 3, 3, 1, 0),
        ("1x1 324->256", 64, 96, 64, 324, 256, 1, 1, 1, 0),
        ("1x1 336->256", 64, 96, 64, 336, 256, 1, 1, 1, 0),
        ("1x1 352->256", 64, 96, 64, 352, 256, 1, 1, 1, 0),
        ("1x1 256->576", 64, 96, 64, 256, 576, 1, 1, 1, 0),
    ]
    TILES = [0, 16128064, 32128128, 32128064]
if os.environ.get("CONV_BENCH_WINO"):    # the fused Winograd F(2x2,3x3) kernel (tile 1) against the direct kernel on the update block's 3x3 layers
    SHAPES = [
        ("3x3 256->192", 64, 64, 96, 256, 192, 3, 3, 1, 0),
        ("3x3 128->256", 64, 64, 96, 128, 256, 3, 3, 1, 0),
        ("3x3 256->126", 64, 64, 96, 256, 126, 3, 3, 1, 0),
        ("3x3 128->64", 64, 64, 96, 128, 64, 3, 3, 1, 0),
    ]
    TILES = [0, 1]
if os.environ.get("CONV_BENCH_WINO4"):   # F(4x4,3x3) (tile 2) against F(2x2,3x3) (tile 1) on the update block's 3x3 layers over the batch: the gate
    SHAPES = [(f"B{b} 3x3 {ci}->{co}", b, 64, 96, ci, co, 3, 3, 1, 0)
              for ci, co in ((256, 192), (128, 256), (256, 126), (128, 64)) for b in (4, 8, 16, 24, 64)]
    TILES = [1, 2]
if os.environ.get("CONV_BENCH_WINO_ENC"):   # ... and on the encoders' stride-1 3x3 layers (65 images) with the epilogues they run, and mask.0
    # 11th field, the epilogue: relu (cnet conv1, mask.0), res (cnet conv2: relu, then relu(y + res)), stats (fnet conv1: identity with
    # the instance-norm partial sums, ofx_conv2d_stats), norm+stats (fnet conv2: relu(norm(x)) on the operand, partial sums)
    SHAPES = [(f"enc 3x3 {c}->{c} @1/{s} {e}", 65, H, W, c, c, 3, 3, 1, 0, e)
              for c, s, H, W in ((64, 2, 384, 256), (96, 4, 192, 128), (128, 8, 96, 64)) for e in ("relu", "res", "stats", "norm+stats")]
    SHAPES.append(("mask.0 3x3 128->256", 64, 64, 96, 128, 256, 3, 3, 1, 0))
    TILES = [0, 1]
if os.environ.get("CONV_BENCH_WINO4_ENC"):  # F(4x4,3x3) (tile 2: the plain kernel and its fused variants) against F(2x2,3x3) (tile 1) on the
    # encoders' three stages over the batch, with the epilogues they run there: the gate of plan path 4
    SHAPES = [(f"B{b} enc {c}->{c} {H}x{W} {e}", b, H, W, c, c, 3, 3, 1, 0, e)
              for c, H, W in ((64, 384, 256), (96, 192, 128), (128, 96, 64)) for e in ("relu", "norm+stats", "res") for b in (4, 8, 16, 64)]
    TILES = [1, 2]
if os.environ.get('CONV_BENCH_TILES'):
    TILES = [int(t) for t in os.environ['CONV_BENCH_TILES'].split(',')]
if os.environ.get("CONV_BENCH_ONLY"):
    SHAPES = [x for x in SHAPES if os.environ["CONV_BENCH_ONLY"] in x[0]]


NAME_W = max([24] + [len(x[0]) for x in SHAPES])   # (24: the layout of the committed tables; the encoder gate's names are longer)


def run(libpath):
    lib = C.CDLL(libpath)
    lib.ofx_conv2d.restype = C.c_int
    lib.ofx_conv2d.argtypes = [C.POINTER(_lib.ConvDesc), C.c_void_p]
    lib.ofx_conv2d_stats.restype = C.c_int
    lib.ofx_conv2d_stats.argtypes = [C.POINTER(_lib.ConvDesc), C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.c_void_p]
    print("==", os.path.basename(libpath))
    for name, B, H, W, ci, co, kh, kw, st, _, *epi in SHAPES:
      epi = epi[0] if epi else "relu"
      for tile in TILES:
            x = torch.randn((B, H, W, ci), device="cuda")
            if os.environ.get("CONV_BENCH_ZERO"):       # power probe: same instruction stream on all-zero operands
                x.zero_()
            K = kh * kw * ci
            Kp = (K + 31) // 32 * 32
            w = torch.randn((co, Kp), device="cuda") * 0.02
            if os.environ.get("CONV_BENCH_ZERO"):
                w.zero_()
            out = torch.empty((B, H // st, W // st, co), device="cuda")
            d = _lib.ConvDesc()
            d.in0, d.ld0, d.c0 = x.data_ptr(), ci, ci
            d.w = w.data_ptr(); d.out = out.data_ptr(); d.ldo = co
            if tile == 1:   # Winograd operand of a 3x3 weight with the same random statistics
                from sd_animation_optical_flow_amd import ops
                u = ops.wino_conv_weight(torch.randn((co, ci, 3, 3)) * 0.02).cuda()
                d.wino_w = u.data_ptr()
            if tile == 2:   # ... and the F(4x4,3x3) operand
                from sd_animation_optical_flow_amd import ops
                u = ops.wino44_conv_weight(torch.randn((co, ci, 3, 3)) * 0.02).cuda()
                d.wino4_w = u.data_ptr()
            d.B, d.Hin, d.Win, d.Hout, d.Wout, d.Cout = B, H, W, H // st, W // st, co
            d.KH, d.KW, d.stride, d.padH, d.padW = kh, kw, st, kh // 2, kw // 2
            d.act, d.epi, d.tile = (0 if "stats" in epi else 1), 0, tile
            keep = []   # buffers the descriptor points at
            if epi == "res":
                r = torch.randn_like(out)
                keep.append(r)
                d.res, d.ldres = r.data_ptr(), co
            if "norm" in epi:
                m, rs = torch.zeros((B, ci), device="cuda"), torch.ones((B, ci), device="cuda")
                keep += [m, rs]
                d.nmean, d.nrstd = m.data_ptr(), rs.data_ptr()
            part = torch.empty((B * H * W * co // 16 + 4096,), device="cuda") if "stats" in epi else None   # room for the direct kernels' rows too
            rows = C.c_int(0)
            d.precision = int(os.environ.get('CONV_BENCH_PREC', '0'))
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            call = (lambda: lib.ofx_conv2d_stats(C.byref(d), part.data_ptr(), part.numel(), C.byref(rows), s)) if part is not None \
                else (lambda: lib.ofx_conv2d(C.byref(d), s))
            for _ in range(3):
                assert call() == 0
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = int(os.environ.get('CONV_BENCH_REPS', '10'))
            e0.record()
            for _ in range(n):
                call()
            e1.record(); torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / n
            fl = 2.0 * B * (H // st) * (W // st) * co * K   # direct-convolution FLOPs for every tile (Winograd: "effective" rate)
            extra = f"  stats rows {rows.value}" if part is not None else ""
            print(f"  {name:<{NAME_W}} tile {tile:>9} {ms:8.3f} ms  {fl / ms / 1e9:7.1f} TFLOP/s{extra}")
if __name__ == "__main__":
    libs = sys.argv[1:] or [_lib.LIB_PATH]
    for l in libs:
        run(l)
