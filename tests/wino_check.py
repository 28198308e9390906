"""Float64 references and an operand-scaled error bound for the convolution tests (not a conftest: imported by name).

A float32 convolution's rounding error at an output is bounded by a multiple of the unit round-off times the magnitude of the
operation, M = conv(|x|, |w|) |scale| + |shift| + |addend|: Winograd transforms add and scale inputs and products before they
cancel, so their error follows the input's magnitude, not the output's.  The check is |out - ref| <= K 2^-24 M + TINY with one K
per kernel.
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24
TINY = 1e-30
# K per kernel: at most 2x the largest |err| / (2^-24 M) measured on MI355X over tests/test_gpu_conv_winograd_sweep.py (the plain
# sweep, the engine-layer and the GRU cases; the direct kernel over the same cases).  Measured maxima:
#   direct (fp32 MFMA kernels)                5.83
#   F(2x2,3x3)                                3.17
#   F(4,5) plain                              21.5
#   F(4,5) GRU_ZR / GRU_Q (pre-activation)    15.7 / 16.1
# The direct kernels' GRU gate epilogues over the cases of tests/gru_check.py (test_gpu_conv_gru_direct.py), measured on MI355X:
#   fp32, every tile / schedule / split-K      2.85  (inside the 5.83 above: K_DIRECT as it stands)
#   bf16x3 / bf16x3_w                          1.94  against the float64 sum of the three products of the CPU-split operands
#   bf16x6 / bf16x6_w                          2.31  against the float64 convolution of the exact operands
# The split-bf16 kernels' plain epilogue over the cases of tests/bf16_check.py (test_gpu_conv_bf16.py), measured on MI355X; the
# pre-split weight formats gave the ratios of the on-the-fly split at every case (bit-identical wherever the two reach one plan):
#   case                        plan (bf16x3)                         bf16x3 / _w    bf16x6 / _w
#   patch-3x3-128x64            128x64 BK 16 patch                    2.02           3.05
#   patch-1x5-128x128-x2        128x128 BK 16 patch                   2.46           4.85
#   patch-5x1-128x128-x2        128x128 BK 16 patch                   2.52           3.33
#   patch-1x5-seam-128x128-x2   128x128 BK 16 patch                   2.28           3.06
#   patch-over-128x64           128x64 BK 16 patch                    1.87           2.26
#   patch-over-128x128          128x128 BK 16 patch                   2.07           2.80
#   gather-64x64                64x64 BK 16 gather                    1.88           2.60
#   gather-128x64               128x64 BK 16 gather                   1.75           2.46
#   gather-128x128              128x128 BK 16 gather                  1.86           2.41
#   gather-auto                 128x128 BK 16 gather                  2.04           2.80
#   gather-auto-ws              128x128 BK 16 gather                  2.09           3.03
#   small-grid-auto-ws          64x64 BK 16 gather                    2.02           2.08
#   bk32-k324                   128x128 BK 32 gather (others BK 16)   3.24           2.96
#   bk32-3x3-c48                128x128 BK 32 gather (others BK 16)   2.29           2.70
#   stride2-3x3-96              128x128 BK 16 gather                  1.82           2.53
#   stride2-1x1                 64x64 BK 16 gather                    1.54           1.93
#   stem-7x7-s2                 64x64 BK 16 gather                    2.26           2.66
#   convf1-7x7                  64x64 BK 16 gather                    2.67           3.06
#   cout2                       128x128 BK 16 patch                   1.21           1.66
#   out-slice-126               64x64 BK 16 gather                    2.69           3.69
#   out-slice-126-patch         128x128 BK 16 patch                   2.07           3.67
#   epi-scale-shift-res-relu    128x64 BK 16 patch                    1.92           2.36
#   epi-addend-shift            64x64 BK 16 gather                    1.87           2.36
#   epi-tanh-patch              128x128 BK 16 patch                   0.72           1.27
#   epi-sigmoid-gather          64x64 BK 16 gather                    0.24           0.79
#   epi-tanh-gather-128x64      128x64 BK 16 gather                   0.25           0.77
#   norm-gather-relu            64x64 BK 16 gather                    1.50           2.21
#   norm-patch                  128x64 BK 16 patch                    1.83           2.99
#   exact-patch                 128x64 BK 16 patch                    1.13           3.59
#   exact-gather                64x64 BK 16 gather                    1.12           1.77
#   spread-patch                128x128 BK 16 patch                   0.11           0.00
#   spread-gather               128x64 BK 16 gather                   0.22           0.00
#   maximum                                                           3.24           4.85   (4.85: one element of 65536; every other case <= 3.69)
# bf16x3: 3.24 is inside K_DIRECT_BF16X3 = 3.8, which stays as it stands (and keeps the 2x rule: 3.8 <= 2 x 3.24).  bf16x6: 4.85 is above
# the 4.6 the gate cases gave, so the constant moves, to 1.5 x 4.85 and not to the full 2 x: a bf16x6 launch that loses one of its
# 2^-16 / 2^-18 products everywhere stands at 9.9 ... 13 at K = 576 ... 864 (bf16_check.py, mm_dropped / lh_dropped), and a constant
# of 9.7 would leave that no margin.
# What the split-bf16 constants cover is the fp32 accumulation on the bf16 matrix cores; the operand arithmetic is in the reference
# (bf16x6, gate cases: with the three dropped products below 2^-23; bf16_check.py carries them as a derived term of its own).
# K_DIRECT_BF16X6 <= 3 K_DIRECT whatever is measured (fp32-accurate).
# The fp32 kernels' plain epilogue over the cases of tests/fp32_check.py (test_gpu_conv_fp32.py: the 12 fp32 rows of kTiles on every
# schedule, OFX_EPI_PLAIN p- / ks2- / sk / auto- / e- / o- / s-, kEpiPlainT t-, norm on load n-), measured on MI355X against the
# float64 convolution of the exact operands; x2: paired pipelines, split n: split-K:
#   case                       plan                        ratio  | case                       plan                        ratio
#   p-128x128-patch-seam-x2    128x128 BK 16 patch         3.79   | e-addend-shift-gather      128x128 BK 16 gather        3.19
#   p-128x128-patch-over       128x128 BK 16 patch         4.06   | e-addend-shift-patch       128x64 BK 16 patch          4.09
#   p-128x128-scalar-s2        128x128 BK 16 scalar        2.81   | o-slice-126-gather         64x64 BK 32 gather          3.24
#   p-128x128-gather           128x128 BK 16 gather        3.92   | o-slice-126-patch          128x128 BK 16 patch         3.55
#   p-256x64-patch             256x64 BK 16 patch          3.70   | o-slice-126-128x96         128x96 BK 16 patch          3.39
#   p-256x64-patch-over        256x64 BK 16 patch          4.51   | o-slice-126-128x192        128x192 BK 16 gather        3.73
#   p-256x64-scalar-1x1        256x64 BK 16 scalar         3.01   | s-spread-patch             128x64 BK 16 patch          0.20
#   p-256x64-scalar-s2         256x64 BK 16 scalar         3.14   | s-spread-gather            128x128 BK 32 gather        0.41
#   p-256x64-gather            256x64 BK 16 gather         3.29   | s-spread-ks2               64x64 BK 32 x2 scalar       0.18
#   p-128x192-patch-200        128x192 BK 16 patch         3.58   | t-128x128-patch            128x128 BK 16 patch         1.18
#   p-128x192-gather-200       128x192 BK 16 gather        2.94   | t-128x128-gather           128x128 BK 16 gather        0.25
#   p-128x192-gather-x2        128x192 BK 16 gather        3.87   | t-256x64-patch             256x64 BK 16 patch          1.91
#   p-128x96-patch-96          128x96 BK 16 patch          3.90   | t-256x64-scalar            256x64 BK 16 scalar         0.00
#   p-128x96-patch-200         128x96 BK 16 patch          4.33   | t-128x192-patch            128x192 BK 16 patch         1.33
#   p-128x96-gather-96         128x96 BK 16 gather         3.30   | t-128x192-gather           128x192 BK 16 gather        0.61
#   p-128x96-gather-200        128x96 BK 16 gather         3.77   | t-128x96-patch             128x96 BK 16 patch          1.15
#   p-128x96-scalar-s2         128x96 BK 16 scalar         3.69   | t-128x96-scalar            128x96 BK 16 scalar         1.18
#   p-128x64-patch-5x1         128x64 BK 16 patch          3.98   | t-128x64-patch             128x64 BK 16 patch          1.15
#   p-128x64-scalar-x2-s2      128x64 BK 16 scalar         3.00   | t-128x64-gather            128x64 BK 16 gather         1.70
#   p-128x64-gather            128x64 BK 16 gather         3.91   | t-128x128k32-scalar        128x128 BK 32 scalar        1.11
#   p-128x128k32-scalar-x2     128x128 BK 32 scalar        3.36   | t-128x64k32-gather         128x64 BK 32 gather         0.69
#   p-128x128k32-k324          128x128 BK 32 gather        3.47   | t-128x32-scalar            128x32 BK 32 scalar         0.94
#   p-128x128k32-c48           128x128 BK 32 gather        3.82   | t-64x64k16-gather          64x64 BK 16 gather          0.00
#   p-128x64k32-scalar         128x64 BK 32 scalar         3.67   | t-64x64-patch              64x64 BK 32 patch           1.65
#   p-128x64k32-k324           128x64 BK 32 gather         4.45   | t-64x64-scalar             64x64 BK 32 scalar          0.93
#   p-128x32-cout2-scalar      128x32 BK 32 scalar         2.33   | t-ks2-auto                 64x64 BK 32 x2 scalar       2.17
#   p-128x32-cout24-scalar-x2  128x32 BK 32 scalar         3.26   | t-sk3-patch                64x64 BK 32 split 3 patch   1.28
#   p-128x32-cout2-gather      128x32 BK 32 gather         2.04   | t-sk2-gather               64x64 BK 32 split 2 gather  0.88
#   p-128x32-cout24-gather     128x32 BK 32 gather         2.72   | n-128x128-patch            128x128 BK 16 patch         1.73
#   p-64x64k16-scalar          64x64 BK 16 scalar          2.88   | n-128x128-scalar           128x128 BK 16 scalar        2.52
#   p-64x64k16-gather          64x64 BK 16 gather          3.07   | n-256x64-patch-over        256x64 BK 16 patch          2.61
#   p-64x64-patch-x2           64x64 BK 32 patch           3.73   | n-256x64-gather            256x64 BK 16 gather         2.38
#   p-64x64-patch-seam         64x64 BK 32 patch           3.19   | n-128x192-patch            128x192 BK 16 patch         2.62
#   p-64x64-scalar             64x64 BK 32 scalar          3.13   | n-128x192-gather           128x192 BK 16 gather        2.01
#   p-64x64-gather             64x64 BK 32 gather          3.17   | n-128x96-patch             128x96 BK 16 patch          3.01
#   ks2-forced-k36             64x64 BK 32 x2 gather       3.12   | n-128x96-gather            128x96 BK 16 gather         3.50
#   ks2-forced-one-chunk       64x64 BK 32 x2 scalar       3.31   | n-128x64-patch             128x64 BK 16 patch          3.83
#   ks2-auto-9-chunks          64x64 BK 32 x2 scalar       1.87   | n-128x64-scalar-1x1        128x64 BK 16 scalar         2.24
#   sk3-patch                  64x64 BK 32 split 3 patch   1.80   | n-128x128k32-gather        128x128 BK 32 gather        2.00
#   sk2-patch                  64x64 BK 32 split 2 patch   2.65   | n-128x64k32-scalar         128x64 BK 32 scalar         3.51
#   sk4-scalar                 64x64 BK 32 split 4 scalar  2.06   | n-128x32-gather            128x32 BK 32 gather         2.02
#   sk2-gather                 64x64 BK 32 split 2 gather  2.26   | n-64x64k16-scalar          64x64 BK 16 scalar          3.02
#   auto-1x1-s2                64x64 BK 32 scalar          2.85   | n-64x64-patch              64x64 BK 32 patch           3.40
#   auto-stem-7x7-s2           64x64 BK 32 gather          2.63   | n-64x64-gather             64x64 BK 32 gather          2.46
#   e-ssrr-patch               128x64 BK 16 patch          2.72   | n-ks2-forced               64x64 BK 32 x2 gather       1.08
#   e-ssrr-gather              64x64 BK 16 gather          2.92   | n-sk3-patch                64x64 BK 32 split 3 patch   1.65
#   e-ssrr-sk                  64x64 BK 32 split 4 scalar  1.51   | n-sk4-scalar               64x64 BK 32 split 4 scalar  0.39
# maximum 4.51 (p-256x64-patch-over: 3x3 on overhanging 16x16 patches), inside the sweep's 5.83 and K_DIRECT = 11.0, which stays
# as it stands: no constant of its own for this table, the 7x7 stem (196 taps) included at 2.63.  The transcendental cases are
# small because ACT_ULP is taken off first; the spread cases because M >> |ref| by construction.
# The direct kernels off 'same' padding over the cases of tests/geom_check.py (test_gpu_conv_geometry.py: pads, output sizes and strides
# that padH = KH // 2 never reaches, the VAE encoder's Downsample on every fp32 row of kTiles and every fp16 instantiation), measured on
# MI355X with the constants above and below as they stand -- a geometry changes which terms enter a sum, not the arithmetic.  fp32,
# |err| / (slope 2^-24 M) against the float64 convolution of the exact operands (x2: paired pipelines, split n: split-K):
#   case                       plan                        ratio  | case                       plan                        ratio
#   g-valid-gather             128x128 BK 16 gather        4.26   | g-down-256x64-gather       256x64 BK 16 gather         3.32
#   g-valid-scalar             64x64 BK 32 scalar          5.14   | g-down-256x64-scalar       256x64 BK 16 scalar         3.55
#   g-valid-s2-gather          256x64 BK 16 gather         2.68   | g-down-128x192-gather      128x192 BK 16 gather        2.93
#   g-valid-s2-scalar          128x128 BK 16 scalar        3.29   | g-down-128x96-gather       128x96 BK 16 gather         3.85
#   g-valid-s2-R-gather        64x64 BK 32 gather          2.85   | g-down-128x96-scalar       128x96 BK 16 scalar         3.44
#   g-valid-s2-R-scalar        128x64 BK 16 scalar         2.97   | g-down-128x64-gather       128x64 BK 16 gather         3.26
#   g-wide-gather              128x192 BK 16 gather        4.55   | g-down-128x64-scalar       128x64 BK 16 scalar         2.55
#   g-wide-scalar              256x64 BK 16 scalar         5.34   | g-down-128x128k32-gather   128x128 BK 32 gather        3.67
#   g-ring-gather              128x96 BK 16 gather         3.46   | g-down-128x128k32-scalar   128x128 BK 32 scalar        4.01
#   g-ring-scalar              128x64 BK 32 scalar         3.70   | g-down-128x64k32-gather    128x64 BK 32 gather         2.32
#   g-ring-1x1-gather          64x64 BK 16 gather          2.58   | g-down-128x64k32-scalar    128x64 BK 32 scalar         2.97
#   g-ring-1x1-scalar          128x32 BK 32 scalar         3.77   | g-down-128x32-gather       128x32 BK 32 gather         2.58
#   g-asym-h-gather            128x64 BK 16 gather         3.75   | g-down-128x32-scalar       128x32 BK 32 scalar         3.43
#   g-asym-h-scalar            128x96 BK 16 scalar         4.51   | g-down-64x64k16-gather     64x64 BK 16 gather          3.40
#   g-asym-w-gather            128x128 BK 32 gather        3.94   | g-down-64x64k16-scalar     64x64 BK 16 scalar          3.78
#   g-asym-w-scalar            64x64 BK 16 scalar          4.07   | g-down-64x64x2-gather      64x64 BK 32 x2 gather       2.79
#   g-valid-1x5-gather         128x64 BK 32 gather         3.32   | g-down-64x64x2-scalar      64x64 BK 32 x2 scalar       2.24
#   g-valid-1x5-scalar         128x128 BK 32 scalar        3.57   | g-down-64x64-gather        64x64 BK 32 gather          3.14
#   g-valid-5x1-gather         128x32 BK 32 gather         3.16   | g-down-64x64-scalar        64x64 BK 32 scalar          4.93
#   g-valid-5x1-scalar         64x64 BK 32 x2 scalar       2.05   | g-down-64x64sk-gather      64x64 BK 32 split 2 gather  4.19
#   g-crop-gather              64x64 BK 32 x2 gather       2.50   | g-down-64x64sk-scalar      64x64 BK 32 split 3 scalar  1.81
#   g-crop-scalar              128x64 BK 16 scalar         3.22   | g-down-norm-gather         128x64 BK 16 gather         2.92
#   g-over-gather              64x64 BK 16 gather          4.04   | g-down-norm-scalar         64x64 BK 32 scalar          1.54
#   g-over-scalar              128x128 BK 16 scalar        3.70   | g-down-slice               128x128 BK 16 scalar        3.77
#   g-down-x2                  128x128 BK 32 scalar        3.41   | g-down-tanh                64x64 BK 16 gather          1.11
#   g-valid-x2                 128x64 BK 16 scalar         3.24   | g-down-ssrr                128x64 BK 32 scalar         2.42
#   g-wide-x2                  64x64 BK 32 scalar          4.05   | g-valid-addend-shift       128x96 BK 16 scalar         3.92
#   g-down-128x128-gather      128x128 BK 16 gather        3.01   | g-model-fp32               64x64 BK 32 x2 scalar       2.03
#   g-down-128x128-scalar      128x128 BK 16 scalar        4.49   |
# maximum 5.34 (g-wide-scalar: 3x3, pad (2, 2), out (H + 2, W + 2) on two 256-row tiles), inside the sweep's 5.83 and K_DIRECT = 11.0.
# fp16 (OFX_PREC_F16; the norm cases OFX_PREC_F16_EPI), |err| / f16_check's derived bound, which is 1 at the bound:
#   case                               plan                  ratio  | case                               plan                  ratio
#   g-f16-valid-gather                 64x64 BK 32 gather    0.032  | g-f16-crop-scalar                  64x64 BK 32 scalar    0.002
#   g-f16-valid-scalar                 64x64 BK 32 scalar    0.003  | g-f16-over-gather                  64x64 BK 32 gather    0.036
#   g-f16-valid-s2-gather              64x64 BK 32 gather    0.030  | g-f16-over-scalar                  64x64 BK 32 scalar    0.002
#   g-f16-valid-s2-scalar              64x64 BK 32 scalar    0.002  | g-f16-down-128x128-bk16-gather     128x128 BK 16 gather  0.031
#   g-f16-wide-gather                  64x64 BK 32 gather    0.038  | g-f16-down-128x128-bk16-scalar     128x128 BK 16 scalar  0.002
#   g-f16-wide-scalar                  64x64 BK 32 scalar    0.002  | g-f16-down-128x128-bk32-gather     128x128 BK 32 gather  0.027
#   g-f16-ring-gather                  64x64 BK 32 gather    0.046  | g-f16-down-128x128-bk32-scalar     128x128 BK 32 scalar  0.002
#   g-f16-ring-scalar                  64x64 BK 32 scalar    0.002  | g-f16-down-128x64-bk16-gather      128x64 BK 16 gather   0.032
#   g-f16-ring-1x1-gather              64x64 BK 32 gather    0.261  | g-f16-down-128x64-bk16-scalar      128x64 BK 16 scalar   0.003
#   g-f16-ring-1x1-scalar              64x64 BK 32 scalar    0.020  | g-f16-down-128x64-bk32-gather      128x64 BK 32 gather   0.028
#   g-f16-asym-h-gather                64x64 BK 32 gather    0.035  | g-f16-down-128x64-bk32-scalar      128x64 BK 32 scalar   0.004
#   g-f16-asym-h-scalar                64x64 BK 32 scalar    0.002  | g-f16-down-64x64-bk16-gather       64x64 BK 16 gather    0.039
#   g-f16-asym-w-gather                64x64 BK 32 gather    0.043  | g-f16-down-64x64-bk16-scalar       64x64 BK 16 scalar    0.004
#   g-f16-asym-w-scalar                64x64 BK 32 scalar    0.002  | g-f16-down-64x64-bk32-gather       64x64 BK 32 gather    0.041
#   g-f16-valid-1x5-gather             64x64 BK 32 gather    0.059  | g-f16-down-64x64-bk32-scalar       64x64 BK 32 scalar    0.004
#   g-f16-valid-1x5-scalar             64x64 BK 32 scalar    0.006  | g-f16-down-norm-gather             128x64 BK 32 gather   0.014
#   g-f16-valid-5x1-gather             64x64 BK 32 gather    0.065  | g-f16-down-norm-scalar             64x64 BK 16 scalar    0.006
#   g-f16-valid-5x1-scalar             64x64 BK 32 scalar    0.005  | g-f16-down-small                   64x64 BK 32 scalar    0.004
#   g-f16-crop-gather                  64x64 BK 32 gather    0.033  | g-f16-model-fp16                   64x64 BK 32 scalar    0.002
# maximum 0.261 (g-f16-ring-1x1-gather: K = 4, where the bound is smallest).  Split bf16, |err| / (2^-24 M); the pre-split weight formats gave the
# ratios of the on-the-fly split at every case (bit-identical wherever the two reach one plan):
#   case                    plan (bf16x3)                         bf16x3 / _w    bf16x6 / _w
#   g-bf16-down-64x64       64x64 BK 16 gather                    1.86           2.01
#   g-bf16-down-128x64      128x64 BK 16 gather                   1.61           2.62
#   g-bf16-down-128x128     128x128 BK 16 gather                  1.86           2.23
#   g-bf16-down-bk32        128x128 BK 32 gather (others BK 16)   2.72           3.04
#   g-bf16-valid-64x64      64x64 BK 16 gather                    2.59           2.52
#   g-bf16-valid-128x64     128x64 BK 16 gather                   2.07           2.37
#   g-bf16-valid-128x128    128x128 BK 16 gather                  1.74           2.56
#   g-bf16-valid-bk32       128x128 BK 32 gather (others BK 16)   2.46           2.73
#   g-bf16-wide-64x64       64x64 BK 16 gather                    3.00           2.84
#   g-bf16-wide-128x64      128x64 BK 16 gather                   1.92           2.66
#   g-bf16-wide-128x128     128x128 BK 16 gather                  2.22           2.67
#   g-bf16-wide-bk32        128x128 BK 32 gather (others BK 16)   2.17           2.50
#   g-bf16-down-norm        64x64 BK 16 gather                    1.05           2.92
#   maximum                                                       3.00           3.04   (inside K_DIRECT_BF16X3 = 3.8 and K_DIRECT_BF16X6 = 7.3)
# Every output with no tap inside the image (the frame of `ring` / `ring-1x1`, the rows and columns of `over` beyond the natural
# output) came out as the epilogue of an exact zero, bit for bit, in all three arithmetics.  No kernel defect found.
K_DIRECT = 11.0
K_DIRECT_BF16X3 = 3.8
K_DIRECT_BF16X6 = 7.3    # measured maximum 4.85
K_F23 = 6.0
K_F45 = 42.0
K_F45_GRU = 32.0
# the sweep's worst fused ratio over its worst direct ratio, per algorithm (measured: 3x3 0.48, 1x5 3.92, 5x1 3.63)
K_SAME_SCALE = 7.5
ACT_ULP = 2e-7           # the activation's own evaluation (ofx_sigmoid / ofx_tanh: __expf and a hardware reciprocal), absolute


def pad_of(kh, kw):
    return (kh // 2, kw // 2)


def conv64(x, w, kh, kw):
    """x NCHW, w OIHW (any float dtype) -> the 'same' correlation in float64."""
    return F.conv2d(x.double(), w.double().view(w.shape[0], -1, kh, kw), padding=pad_of(kh, kw))


def geometry_of(c):
    """A case's (padH, padW), (Hout, Wout) (ofx_conv_desc, include/ofx.h).  The optional keys `pad` and `out_hw` give them; the default
    is 'same' padding k // 2 and the output size that follows.  Filters: `kh` / `kw`, or a square `k`."""
    kh, kw = c.get("kh", c.get("k")), c.get("kw", c.get("k"))
    ph, pw = c.get("pad") or (kh // 2, kw // 2)
    natural = ((c["H"] + 2 * ph - kh) // c["stride"] + 1, (c["W"] + 2 * pw - kw) // c["stride"] + 1)
    return (ph, pw), tuple(c.get("out_hw") or natural)


def pad_amounts(hin, win, kh, kw, stride, pad, out_hw):
    """(top, bottom, left, right) rows / columns of zeros around an image: `pad` above and left, below and right as many as the last
    output needs, (Hout - 1) stride + KH - padH - Hin clamped at 0."""
    (ph, pw), (ho, wo) = pad, out_hw
    return ph, max((ho - 1) * stride + kh - ph - hin, 0), pw, max((wo - 1) * stride + kw - pw - win, 0)


def pad_nhwc(x, amounts):
    top, bottom, left, right = amounts
    return F.pad(x, (0, 0, left, right, top, bottom))


def conv64_geometry(x, w, stride, pad, out_hw, padded=False):
    """x NHWC, w OIHW (any float dtype) -> the float64 convolution of a descriptor's geometry, NHWC: out[b, oy, ox, n] sums
    x[b, oy stride - padH + ky, ox stride - padW + kx, c] w[n, c, ky, kx], taps outside the image zero.  Zero-pad, F.conv2d with no
    padding, crop to [:Hout, :Wout].  padded: x already carries pad_amounts' zeros (or whatever a simulated bug put there)."""
    kh, kw = w.shape[2:]
    if not padded:
        x = pad_nhwc(x, pad_amounts(x.shape[1], x.shape[2], kh, kw, stride, pad, out_hw))
    out = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), stride=stride)
    assert out.shape[2] >= out_hw[0] and out.shape[3] >= out_hw[1]
    return out[:, :, :out_hw[0], :out_hw[1]].permute(0, 2, 3, 1)


def _chan(v):
    return v.double().view(1, -1, 1, 1)


def reference(x, w, kh, kw, scale=None, shift=None, addend=None, relu=False):
    """The plain epilogue in float64 and its magnitude M (both NCHW).  addend NCHW."""
    acc = conv64(x, w, kh, kw)
    mag = conv64(x.abs(), w.abs(), kh, kw)
    if scale is not None:
        acc, mag = acc * _chan(scale), mag * _chan(scale).abs()
    if shift is not None:
        acc, mag = acc + _chan(shift), mag + _chan(shift).abs()
    if addend is not None:
        acc, mag = acc + addend.double(), mag + addend.double().abs()
    return (torch.relu(acc) if relu else acc), mag


def violations(out, ref, mag, K, slope=1.0, extra=0.0):
    """Mask of the elements outside |out - ref| <= slope (K 2^-24 M) + extra + TINY (NaN counts as outside)."""
    err = (out.double() - ref.double()).abs()
    return ~(err <= slope * K * EPS * mag.double() + extra + TINY)


def worst_ratio(out, ref, mag, slope=1.0, extra=0.0):
    """max over the elements of (|out - ref| - extra) / (slope 2^-24 M): the smallest K the elements satisfy."""
    err = (out.double() - ref.double()).abs() - extra
    r = err.clamp_min(0) / (slope * EPS * mag.double()).clamp_min(TINY)
    return float(r.max()) if r.numel() else 0.0


def check(out, ref, mag, K, what, slope=1.0, extra=0.0):
    """Assert the bound and return the worst ratio."""
    bad = violations(out, ref, mag, K, slope, extra)
    ratio = worst_ratio(out, ref, mag, slope, extra)
    if bool(bad.any()):
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside K = {K} (worst ratio {ratio:.3g}); "
                             f"first at {idx}: got {float(out[tuple(idx)])}, want {float(ref[tuple(idx)])}")
    return ratio
