"""Shapes of the `-m gpu` oracle-parity cases, as data.

tests/test_kernels_gpu.py and tests/test_model_gpu.py parametrise over these lists; tests/test_dispatch_coverage.py
(CPU) asks the library's dry-run dispatch which kernel instantiation every case runs and asserts that every
instantiation the BASELINE configurations launch at full size appears among them.  A case belongs here only if its GPU
test compares the kernel with the CPU oracle / an fp64 restatement (not with another device kernel).
"""
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
HALF_DTYPES = [BF16, F16]

# ---- x3d_pw_fwd: N, Cin, Cout, T, H, W, stride, prologue ------------------------------------------------------------
PW_FWD = [
    (2, 48, 108, 2, 5, 13, 1, None), (1, 108, 48, 1, 3, 43, 1, "swish"),   # P = 130 / 129: a row's partial 16-byte vector is vector 0 of a 128-point tile (fp32 pipelined kernel: early start in front of the tile)
    (2, 24, 54, 4, 12, 12, 1, None),       # bottleneck a (stage 2 widths)
    (2, 54, 24, 3, 10, 10, 1, "swish"),    # bottleneck c with BN_b + SE gate + swish folded
    (2, 24, 48, 4, 12, 12, 2, None),       # strided shortcut (valid, samples pixels 0,2,..)
    (1, 48, 108, 13, 5, 5, 1, "relu"),     # P = 325 (odd): scalar path
    (2, 96, 216, 2, 7, 7, 1, None),        # Cout > 128: two row blocks
    (1, 216, 96, 2, 7, 7, 1, "swish"),     # K chunking (does not fit LDS resident)
    (1, 24, 24, 2, 9, 11, 2, None),        # odd extents with stride 2
    (1, 200, 40, 1, 4, 8, 1, "swish"),     # widths off the 32-grid
    (1, 24, 48, 2, 56, 56, 2, None), (2, 48, 96, 2, 28, 28, 2, None), (2, 96, 192, 4, 14, 14, 2, None),  # gather groups 4 / 2 / 1
    (1, 24, 24, 2, 32, 32, 2, None),       # Wo % 8 == 0
    (2, 432, 192, 2, 8, 8, 1, "swish"), (2, 192, 432, 2, 8, 8, 1, None), (1, 440, 200, 1, 8, 5, 1, "relu"),  # weights-streamed / -stationary paths
    (2, 216, 96, 2, 14, 14, 1, "swish"), (2, 96, 216, 2, 14, 14, 1, None), (2, 200, 90, 1, 8, 8, 1, "relu"),  # stage-4 weights-stationary shapes (two workgroups per CU)
    (2, 96, 432, 2, 14, 14, 1, None),      # stage-5 block 0 `a` conv (7 waves x 2 row blocks x 6 k-steps)
    (1, 24, 24, 1, 156, 156, 2, None), (1, 24, 48, 1, 78, 78, 2, None), (1, 48, 96, 2, 39, 39, 2, None),   # X3D-L / XL shortcuts
    (1, 96, 192, 2, 20, 20, 2, None),
    (1, 96, 192, 8, 14, 14, 2, None), (1, 24, 48, 8, 78, 78, 2, None),   # odd Wo with P % 8 == 0: gather group 1 on the vector path
    (1, 24, 24, 8, 156, 156, 2, None),                                   # Wo = 78: gather group 2
    (1, 24, 54, 1, 32, 32, 1, None), (1, 108, 48, 1, 16, 16, 1, "swish"), (1, 48, 108, 1, 16, 16, 1, None),  # aligned stage-2/3 layers
    (1, 24, 108, 1, 16, 16, 1, None), (1, 48, 216, 1, 16, 16, 1, None),
    # X3D-S stages 4 / 5 (13 frames: rows of 1300 / 325 points, not multiples of 8): 16-bit storage takes the vector kernels
    # with ragged row ends (unaligned row starts, a row's last vector element by element)
    (2, 216, 96, 13, 10, 10, 1, "swish"), (2, 96, 216, 13, 10, 10, 1, None), (1, 432, 192, 13, 5, 5, 1, "swish"),
    (1, 192, 432, 13, 5, 5, 1, None), (1, 24, 54, 1, 3, 4, 1, None),   # (... and a row shorter than two vectors: P = 12)
    # strided shortcut with an ODD input width on the vector gather (groups of 4 / 2 / 1, the row's last group loaded early)
    (1, 24, 48, 2, 11, 23, 2, None), (1, 32, 32, 4, 9, 27, 2, None), (1, 24, 48, 8, 13, 13, 2, None),
    # ... whose rows are ONE gather group wide (7 -> 4, 3 -> 2: stage 5 of 112-pixel crops): the early load of the last
    # group would start before the row (before the tensor for its first row) -- these take the next smaller group
    (1, 96, 192, 8, 7, 7, 2, None), (2, 96, 192, 8, 3, 3, 2, None),
    # round 6: the shortcut convs as DENSE launches on the even-pixel copy of the block input (x3d_subsample2): the compact planes
    # of X3D-XS .. M (40 / 56, 28, 14, 7 wide) and X3D-L / XL (78, 39, 20, 10 wide; 32 -> 32)
    (1, 24, 24, 2, 40, 40, 1, None), (2, 24, 24, 1, 56, 56, 1, None), (1, 24, 48, 2, 28, 28, 1, None), (2, 48, 96, 2, 14, 14, 1, None),
    (2, 96, 192, 4, 7, 7, 1, None), (1, 24, 24, 2, 78, 78, 1, None), (1, 32, 32, 1, 78, 78, 1, None), (1, 24, 48, 2, 39, 39, 1, None),
    (1, 48, 96, 2, 20, 20, 1, None), (1, 96, 192, 2, 10, 10, 1, None),
    # the shipped X3D-S yaml with 16-bit storage (13 frames, 160-pixel crops; tests/test_dispatch_coverage.py
    # test_every_instantiation_of_a_shipped_config_is_covered), at the smallest N and T that keep the instantiation:
    (1, 48, 96, 1, 20, 20, 2, None),       # stage-4 shortcut 20 -> 10: pw_gemm_bf16_kernel<T, 8, 3, 0, 100, 2, 8, 1>
    (1, 96, 432, 1, 10, 10, 1, None),      # stage-5 `a` conv, inference (with a panel): pw_gemm_wst_kernel<T, 0, 100, 7, 2, 6, 2, 1>
]
# ... with the residual tail of the block below folded into the prologue (16-bit storage; prologue "tail": identity shortcut,
# "tail_conv": shortcut conv with its own BN): x = raw c output, in_add = shortcut, in_store = the block output y
PW_FWD_TAIL = [
    (2, 24, 54, 4, 12, 12, 1, "tail"), (1, 48, 108, 2, 16, 16, 1, "tail_conv"), (1, 24, 108, 1, 16, 16, 1, "tail"),   # stages 2 / 3
    (1, 48, 216, 1, 16, 16, 1, "tail"), (1, 32, 72, 1, 16, 16, 1, "tail"), (1, 72, 162, 1, 8, 8, 1, "tail_conv"),     # stage-4 block 0; X3D-XL
    (1, 48, 108, 13, 5, 5, 1, "tail"), (2, 96, 216, 13, 10, 10, 1, "tail_conv"), (1, 24, 54, 1, 3, 4, 1, "tail"),     # odd / ragged point counts
    (3, 40, 72, 2, 7, 8, 1, "tail_conv"),
    (1, 96, 432, 1, 10, 10, 1, "tail"),   # X3D-S stage-5 `a` conv, training, 16-bit (with a panel): pw_gemm_wst_kernel<T, 3, 100, 7, 2, 6, 2, 1>
    # stages 4 / 5: the weights-stationary kernel carries the fold (shapes 4, 5, 2 of pw_gemm_wst.h; with a weight panel), whole and
    # ragged rows (13 frames of 10 x 10 / 5 x 5), two samples, a partial last tile
    (2, 96, 216, 4, 14, 14, 1, "tail"), (1, 96, 432, 2, 14, 14, 1, "tail_conv"), (2, 192, 432, 4, 7, 7, 1, "tail"), (1, 192, 432, 8, 7, 7, 1, "tail_conv"),
    (1, 96, 216, 13, 10, 10, 1, "tail"), (2, 192, 432, 13, 5, 5, 1, "tail_conv"),
    # "tail1": no Add -- the stem's BatchNorm + ReLU folded into the first block's `a` conv (x = raw conv_t output, in_store = y0)
    (2, 24, 54, 2, 16, 16, 1, "tail1"), (1, 32, 72, 1, 16, 16, 1, "tail1"), (1, 24, 54, 1, 3, 4, 1, "tail1"), (2, 24, 54, 13, 5, 5, 1, "tail1"),
]
# X3D-XL widths (configs/kinetics/X3D_XL.yaml: width factor 2.9, bottleneck 2.25): 32/72, 72/162, 136/306, 280/630, conv5 630
PW_FWD_XL = [
    (1, 32, 72, 1, 16, 16, 1, None), (1, 72, 32, 1, 16, 16, 1, "swish"), (1, 32, 32, 1, 16, 16, 2, None),
    (1, 32, 162, 1, 16, 16, 1, None), (1, 162, 72, 1, 8, 8, 1, "swish"), (1, 72, 162, 1, 8, 8, 1, None), (1, 32, 72, 1, 16, 16, 2, None),
    (1, 72, 306, 1, 8, 8, 1, None), (1, 306, 136, 1, 8, 8, 1, "swish"), (1, 136, 306, 1, 8, 8, 1, None), (1, 72, 136, 1, 16, 16, 2, None),
    (1, 136, 630, 1, 8, 8, 1, None), (1, 630, 280, 1, 8, 8, 1, "swish"), (1, 280, 630, 1, 8, 8, 1, None), (1, 136, 280, 1, 16, 16, 2, None),
    (1, 32, 72, 8, 78, 78, 2, None), (1, 32, 32, 8, 156, 156, 2, None),
]

# ---- x3d_pw_fwd with the INFERENCE epilogue (folded BN + residual Add + ReLU on the accumulators): the stride-1 cases above
# that carry the `c` conv's prologue, with the shortcut alternating between the block input ("identity") and a raw
# shortcut-conv output with its own BN ("conv"); plus plain BN (+ ReLU) epilogues without a residual.
#   N, Cin, Cout, T, H, W, prologue, residual, out_act
PW_FWD_INFER = [(n, ci, co, t, h, w, pro, ("identity", "conv")[i % 2], "relu")
                for i, (n, ci, co, t, h, w, st, pro) in enumerate(PW_FWD + PW_FWD_XL) if st == 1 and pro == "swish"] + [
    (2, 24, 54, 4, 12, 12, None, None, "relu"), (1, 48, 108, 13, 5, 5, "relu", None, None), (2, 192, 432, 2, 8, 8, None, "identity", None),
    (2, 96, 216, 2, 14, 14, None, None, "relu"), (1, 280, 630, 1, 8, 8, None, "conv", "relu"),
    (1, 54, 24, 2, 20, 20, "swish", "identity", "relu"), (1, 108, 48, 2, 10, 10, "swish", "conv", "relu"),   # fp32 panels of 1 / 2 row tiles
    (1, 216, 96, 2, 10, 10, "swish", "identity", "relu"), (1, 432, 192, 4, 5, 5, "swish", "identity", "relu"),   # ... 3 / 4 (X3D-XS, config 1)
]

# ---- x3d_pw_dgrad: N, Cin, Cout, T, H, W  x  epilogue -----------------------------------------------------------------
PW_DGRAD = [
    (2, 48, 108, 2, 5, 13), (1, 108, 48, 1, 3, 43),   # P = 130 / 129 (see PW_FWD)
    (2, 24, 54, 4, 12, 12), (1, 54, 24, 3, 10, 10), (1, 48, 108, 13, 5, 5), (1, 96, 216, 2, 7, 7),
    (1, 216, 96, 2, 7, 7), (1, 200, 40, 1, 4, 8),
    (1, 54, 24, 4, 14, 14), (1, 48, 108, 2, 28, 28),   # strided add with rows of 2k / 4k points (pair / quad groups)
    (1, 192, 432, 2, 8, 8), (1, 432, 192, 2, 8, 8), (1, 96, 192, 2, 8, 8), (1, 96, 432, 2, 14, 14),   # stage-5 weights-stationary dgrads
    (1, 24, 48, 1, 16, 16), (1, 48, 96, 1, 16, 16), (1, 48, 216, 1, 16, 16),
    (2, 96, 216, 13, 10, 10), (1, 192, 432, 13, 5, 5), (1, 96, 432, 13, 10, 10), (1, 432, 192, 13, 5, 5),   # X3D-S stages 4 / 5: ragged rows
]
PW_DGRAD_EPI = ["store", "add", "add_strided", "swish_bwd"]

# ---- x3d_pw_wgrad: N, Cin, Cout, T, H, W, stride, prologue --------------------------------------------------------------
PW_WGRAD = [
    (1, 32, 32, 1, 2, 17, 1, None), (2, 48, 108, 1, 33, 2, 1, "swish"),   # P = 34 / 66: the partial vector is vector 0 of the last 32-point step
    (2, 24, 54, 4, 12, 12, 1, None), (2, 54, 24, 3, 10, 10, 1, "swish"), (2, 24, 48, 4, 12, 12, 2, None),
    (1, 48, 108, 13, 5, 5, 1, None), (1, 96, 216, 2, 7, 7, 1, None), (1, 216, 96, 2, 7, 7, 1, "swish"),
    (1, 192, 432, 1, 7, 7, 1, None), (1, 432, 192, 1, 7, 7, 1, "swish"), (1, 24, 24, 2, 9, 11, 2, None),
    (1, 24, 48, 2, 56, 56, 2, None), (2, 48, 96, 2, 28, 28, 2, None), (2, 96, 192, 4, 14, 14, 2, None),  # gather groups 4 / 2 / 1
    (2, 96, 216, 2, 8, 8, 1, None), (2, 192, 432, 3, 8, 8, 1, None), (2, 432, 192, 2, 8, 8, 1, "swish"),  # wide layers: 12-tile groups (4x3 / 3x4)
    (2, 192, 432, 8, 7, 7, 1, None), (3, 432, 192, 8, 7, 7, 1, "swish"), (2, 96, 216, 2, 14, 14, 1, None),  # ragged last 64-point step
    (1, 24, 24, 2, 32, 32, 2, None), (1, 48, 216, 1, 16, 16, 1, None), (1, 24, 24, 1, 156, 156, 2, None),
    (1, 24, 48, 1, 78, 78, 2, None), (1, 48, 96, 2, 39, 39, 2, None), (1, 96, 192, 2, 20, 20, 2, None),
    (1, 96, 192, 8, 14, 14, 2, None), (1, 24, 48, 8, 78, 78, 2, None), (1, 24, 24, 8, 156, 156, 2, None),
    (1, 48, 108, 1, 16, 16, 1, None), (1, 108, 48, 1, 16, 16, 1, "swish"),
    (2, 24, 108, 3, 12, 12, 1, None), (1, 24, 216, 2, 10, 10, 1, None), (2, 54, 24, 13, 10, 10, 1, "swish"),   # fp32 tile groups 4x1 / 8x1 / 1x2 with several point chunks
    (2, 96, 216, 13, 10, 10, 1, None), (2, 216, 96, 13, 10, 10, 1, "swish"), (1, 192, 432, 13, 5, 5, 1, None),   # X3D-S stages 4 / 5: ragged rows
    (1, 432, 192, 13, 5, 5, 1, "swish"),
    (1, 24, 48, 2, 11, 23, 2, None), (1, 32, 32, 4, 9, 27, 2, None), (1, 24, 48, 8, 13, 13, 2, None),   # strided, odd input width: vector gather
    (1, 96, 192, 8, 7, 7, 2, None), (2, 96, 192, 8, 3, 3, 2, None),   # rows one gather group wide (7 -> 4, 3 -> 2)
    # round 6: the shortcut convs' weight gradient as a dense launch on the even-pixel copy (x3d_subsample2)
    (1, 24, 24, 2, 40, 40, 1, None), (2, 24, 24, 1, 56, 56, 1, None), (1, 24, 48, 2, 28, 28, 1, None), (2, 48, 96, 2, 14, 14, 1, None),
    (2, 96, 192, 4, 7, 7, 1, None), (1, 24, 48, 2, 39, 39, 1, None), (1, 48, 96, 2, 20, 20, 1, None), (1, 96, 192, 2, 10, 10, 1, None),
    (2, 48, 96, 13, 10, 10, 1, None), (2, 24, 24, 13, 40, 40, 1, None),
    # the shipped yamls outside the BASELINE plans (tests/test_dispatch_coverage.py), smallest N and T that keep the instantiation
    (1, 48, 96, 1, 20, 20, 2, None),          # X3D-S 16-bit, stage-4 shortcut: pw_wgrad_bf16_v2_kernel<T, 4, 2, 0, 2, 256, 1>
    (1, 162, 72, 4, 39, 39, 1, "swish"),      # X3D-XL fp32 training: pw_wgrad_f32p_kernel<2, 3, 1, 0> (T = 4: below it another point split)
    (1, 280, 630, 1, 10, 10, 1, None),        # ... pw_wgrad_f32p_kernel<2, 4, 0, 0>
    (1, 72, 32, 1, 78, 78, 1, "swish"),       # ... pw_wgrad_f32p_kernel<1, 3, 1, 0>
    (1, 72, 136, 1, 39, 39, 2, None),         # ... pw_wgrad_kernel<float, 1, 4, 0, 1>
]

# ---- fp32 launches whose instantiation only exists at full size: the pipelined fp32 kernels hand tensors their 32-bit buffer
# offsets cannot span (N max(Cin, Cout) + 256 rows of P floats reach 2 GB) to the resident-weights kernels (pw_gemm_f32r.h /
# pw_wgrad_f32r.h), so no smaller N or T keeps the name.
# tests/test_kernels_gpu.py test_pw_f32_past_buffer_offsets_fp64 checks them against fp64 on the GPU, sample by sample.
#   entry, (N, Cin, Cout, T, H, W)
PW_F32_FULL = [
    ("fwd", (21, 24, 54, 16, 156, 156)),      # X3D-L fp32 inference, 24 clips (stage-2 `a` conv): pw_f32r_kernel<4, 2, 4, 0, 100>; N >= 21 at T = 16
    ("wgrad", (16, 32, 72, 16, 156, 156)),    # X3D-XL fp32 training, 16 clips (stage-2 `a` conv): pw_wgrad_f32r_kernel<2, 1, 0>; N = 16 and T = 16 only
]


def pw_f32_full_struct(case):
    entry, (n, cin, cout, t, h, w) = case
    shape = (n, cin, cout, t, h, w, 1, None)
    return pw_fwd_struct(shape, F32, False) if entry == "fwd" else pw_wgrad_struct(shape, F32)

# ---- x3d_pw_bwd (fused dgrad + wgrad): N, Cin, Cout, T, H, W, epilogue ---------------------------------------------------
PW_BWD = [
    (2, 24, 54, 4, 16, 16, "add"), (2, 48, 108, 2, 28, 28, "add"), (1, 24, 108, 3, 16, 16, "add_strided"),
    (2, 24, 54, 2, 28, 28, "add_strided"),     # rows of 28 points: element loads of the shortcut gradient in the epilogue
    (1, 24, 54, 2, 16, 16, "add_strided"),     # rows of 8k points: 8-byte loads (a separate instantiation)
    (2, 54, 24, 4, 16, 16, "swish_bwd"), (2, 108, 48, 3, 12, 12, "swish_bwd"), (3, 40, 20, 1, 7, 8, "swish_bwd"),
    (1, 96, 32, 2, 10, 12, "swish_bwd"),
    (2, 216, 96, 2, 14, 14, "swish_bwd"),      # stage-4 `c` conv: the weights-stationary fused kernel (pw_bwd_wst.hip)
    (24, 216, 96, 8, 14, 14, "swish_bwd"),     # ... several tiles per persistent workgroup, across sample boundaries
    (3, 200, 90, 1, 10, 12, "swish_bwd"),      # ... widths off the grid, a partial last tile per sample (P = 120)
    (1, 200, 40, 2, 8, 8, "add"), (1, 136, 72, 1, 8, 16, "add_strided"),   # sliced `a`-type layers, widths off the grid
    (2, 96, 216, 2, 14, 14, "add"), (24, 96, 216, 8, 14, 14, "add"), (3, 90, 210, 1, 10, 12, "add"),   # stage-4 `a` conv: pw_bwd_wsta.hip
    (1, 32, 72, 1, 16, 16, "add"), (1, 32, 72, 1, 16, 16, "add_strided"), (1, 72, 32, 1, 16, 16, "swish_bwd"),   # X3D-XL stage 2
    # stage-5 `c` conv (432 <-> 192 on 7 x 7 planes): pw_bwd_wst.hip with two slices of seven row blocks over blockIdx.y
    (2, 432, 192, 8, 7, 7, "swish_bwd"), (10, 432, 192, 16, 7, 7, "swish_bwd"), (3, 420, 180, 1, 10, 12, "swish_bwd"),
    (2, 300, 192, 2, 8, 8, "swish_bwd"),       # ... a short second slice (ten row blocks: 7 + 3)
]

# ... without the conv's raw output (pw_bwd_rc.hip: y = W x folded into the BatchNorm backward): N, Cin, Cout, T, H, W, epilogue, tail
PW_BWD_RC = [
    (2, 24, 54, 4, 16, 16, "add", 0), (2, 24, 54, 4, 16, 16, "add", 1), (2, 24, 54, 4, 16, 16, "add", 2),          # stage 2 (X3D-S / M / L)
    (1, 24, 54, 2, 16, 16, "add_strided", 0), (1, 24, 54, 2, 16, 16, "add_strided", 1),                            # block 0 of stage 2 (stem fold = tail 1)
    (2, 24, 54, 2, 28, 28, "add_strided", 0), (2, 24, 54, 2, 28, 28, "add_strided", 2),                            # rows of 28 points: element form
    (1, 24, 108, 3, 16, 16, "add_strided", 0), (1, 24, 108, 3, 16, 16, "add_strided", 1), (1, 24, 108, 3, 16, 16, "add_strided", 2),   # stage 3 block 0
    (1, 24, 108, 2, 12, 12, "add_strided", 2), (1, 24, 108, 2, 12, 12, "add_strided", 1), (2, 24, 54, 2, 28, 28, "add_strided", 1),   # ... X3D-L / XL rows (element form)
    (1, 32, 72, 1, 16, 16, "add", 0), (1, 32, 72, 1, 16, 16, "add", 1), (1, 32, 72, 1, 16, 16, "add_strided", 2),  # X3D-XL stage 2 (Cin = 32: no spare row)
    (3, 20, 40, 1, 7, 8, "add", 1), (1, 24, 20, 2, 10, 12, "add", 2), (2, 8, 31, 1, 9, 8, "add", 0),               # ragged tiles, widths off the grid, Cout + 1 = 32
    (1, 16, 95, 1, 12, 12, "add", 0), (1, 24, 127, 1, 8, 8, "add", 2),                                             # three / four row tiles of g
    (5, 24, 54, 8, 28, 28, "add", 1),                                                                              # several tiles per workgroup, across samples
    (2, 48, 108, 2, 28, 28, "add", 0), (24, 48, 108, 8, 28, 28, "add", 0),                                         # stage 3: two row tiles of x (48 rows in the image)
    (1, 40, 100, 1, 12, 12, "add", 0), (1, 48, 90, 2, 8, 16, "add_strided", 0), (3, 48, 108, 4, 20, 20, "add", 0), # ... widths off the grid, three g tiles, X3D-L planes
    # first `a` conv of stage 4 (48 -> 216: seven row tiles of g, one workgroup per CU): strided add (the model's case, vector and
    # element forms), plain add, several tiles per workgroup across samples, Cout off the grid
    (2, 48, 216, 2, 16, 16, "add_strided", 0), (1, 48, 216, 2, 28, 28, "add_strided", 0), (1, 48, 216, 1, 16, 16, "add", 0),
    (9, 48, 216, 4, 28, 28, "add_strided", 0), (1, 40, 200, 1, 12, 12, "add", 0),
    (1, 48, 216, 8, 13, 13, "add_strided", 0),      # X3D-L / XL: rows of odd length (39 x 39) take the element form of the strided add
    # ... and rows of 4 k + 2 points (78 x 78): element form too (rows of 4 k take the group form: 12, 28, 156)
    (1, 24, 108, 2, 10, 10, "add_strided", 1), (1, 24, 108, 2, 10, 10, "add_strided", 0), (1, 24, 108, 2, 10, 10, "add_strided", 2),
    (1, 24, 54, 2, 6, 14, "add_strided", 1), (2, 24, 54, 2, 9, 8, "add_strided", 0),
]

# ... of the strided shortcut conv (x_stride = 2, epilogue STORE): N, Cin, Cout, T, xH, xW (input extents)
PW_BWD_RC_STRIDED = [
    (2, 24, 24, 4, 32, 32), (2, 24, 24, 2, 112, 112),          # stage 2 (gather groups of 4)
    (1, 24, 48, 4, 28, 28), (1, 24, 48, 2, 56, 56),            # stage 3: rows of 14 outputs (groups of 2) / 28
    (1, 48, 96, 8, 14, 14), (2, 48, 96, 4, 28, 28),            # stage 4: two row tiles of x; rows of 7 outputs (groups of 1)
    (1, 24, 48, 2, 39, 39), (1, 24, 24, 8, 78, 78), (1, 48, 96, 2, 39, 39),
    (1, 24, 24, 2, 12, 156), (1, 24, 48, 8, 6, 78),            # X3D-L stage 2 / 3 rows: 156 -> 78 (groups of 2), 78 -> 39 (groups of 1)            # X3D-L: odd input rows (39 -> 20: the row's last group loaded early)
    (1, 32, 32, 2, 16, 24), (1, 20, 40, 1, 12, 16),            # X3D-XL stage 2 (Cin = Cout = 32), widths off the grid
]

# ... with the residual-tail backward of the block below folded into the epilogue (the `a` convs: ADD epilogues, panels of
# one or two row tiles): N, Cin, Cout, T, H, W, epilogue, tail (1 = identity shortcut below, 2 = shortcut conv below)
PW_BWD_TAIL = [
    (2, 24, 54, 4, 16, 16, "add", 1), (2, 24, 54, 2, 28, 28, "add_strided", 1), (2, 24, 54, 4, 16, 16, "add", 2),   # stage 2 (X3D-S / M / L)
    (1, 24, 54, 2, 16, 16, "add_strided", 1), (1, 24, 54, 2, 16, 16, "add_strided", 2),
    (1, 24, 108, 3, 16, 16, "add_strided", 1), (1, 24, 108, 3, 16, 16, "add_strided", 2),                          # stage 3 block 0
    (1, 24, 108, 2, 12, 12, "add_strided", 1), (1, 24, 108, 2, 12, 12, "add_strided", 2),                          # ... X3D-L / XL rows (78: element form)
    (2, 48, 54, 2, 28, 28, "add", 1), (2, 48, 54, 2, 28, 28, "add", 2),                                            # two row tiles x two dY tiles
    (1, 32, 72, 1, 16, 16, "add", 1), (1, 32, 72, 1, 16, 16, "add", 2), (1, 32, 72, 1, 16, 16, "add_strided", 1),  # X3D-XL stage 2
    (3, 20, 40, 1, 7, 8, "add", 1), (1, 24, 20, 2, 10, 12, "add", 2),                                              # ragged tiles, widths off the grid
    (2, 96, 216, 2, 14, 14, "add", 1), (24, 96, 216, 8, 14, 14, "add", 1), (3, 90, 210, 1, 10, 12, "add", 1),      # stage-4 `a` conv (pw_bwd_wsta.hip)
]

# ---- x3d_dw3d_fwd / x3d_dw3d_bwd: N, C, T, H, W, stride --------------------------------------------------------------------
DW = [
    (2, 5, 4, 16, 16, 1), (2, 5, 4, 16, 16, 2),       # even, SW=2
    (1, 3, 3, 7, 7, 1), (1, 3, 3, 14, 14, 2),         # 7x7 planes, SW=1
    (1, 2, 5, 39, 39, 2), (1, 2, 2, 20, 20, 1),       # X3D-L odd case 39 -> 20 (pads 1/1)
    (2, 3, 5, 39, 39, 1), (1, 2, 4, 78, 78, 2), (1, 3, 3, 25, 37, 1), (1, 2, 2, 41, 43, 1),   # odd row length of 16-bit outputs, strips of four: every second row starts 2 mod 4, several samples / channels (the plane is an odd number of elements: the parity alternates), last strip of 3 / 1 / 3 outputs
    (1, 2, 3, 56, 56, 1), (1, 2, 3, 112, 112, 2),     # X3D-M stage-2 planes, SW=4, H-tiled
    (1, 2, 1, 9, 23, 2), (1, 1, 2, 10, 13, 1),        # T=1 / non-square / odd widths
    (1, 2, 16, 28, 28, 1),                            # vec 4 path for bf16
    (2, 3, 16, 14, 14, 1), (1, 2, 6, 7, 7, 1),        # deep-prefetch variants (dw_pd.hip): T = 4k, T % 4 != 0,
    (1, 2, 1, 7, 7, 1), (1, 2, 7, 12, 12, 2),         #   T < depth, stride 2
    (1, 2, 4, 28, 28, 2),                             # X3D-M stage-4 first block (216 ch 28 -> 14): <2, 2, 2, 4> in bf16
    (1, 2, 3, 56, 56, 2),                             # X3D-M stage-3 first block (56 -> 28)
    # dw3d_bwd_s2_kernel (dw_s2.hip; 16-bit storage, rows of whole 16-byte vectors): T loop unrolled by 6 (T = 6 / 7 / 13 / 16 / 2 / 1),
    # several samples and channels, a partial last H-tile, non-square planes, odd H (one pad row on top)
    (2, 3, 7, 112, 112, 2), (1, 2, 13, 56, 56, 2), (1, 2, 16, 48, 48, 2), (2, 2, 6, 64, 40, 2), (1, 3, 2, 96, 112, 2), (1, 2, 1, 56, 56, 2),
    (1, 2, 8, 45, 48, 2),
    (1, 2, 7, 120, 120, 2),   # planes too large for the ring kernel's constant LDS strides: dw3d_bwd_s2_kernel (two barriers per plane)
    # dw3d_bwd_s1r_kernel (dw_s1.hip; stride 1, strips of four, 16-bit storage): every T mod 6 of the unrolled loop and its drain,
    # several samples / channels, a partial last H-tile, non-square planes
    (2, 3, 7, 56, 56, 1), (1, 2, 13, 40, 40, 1), (1, 2, 16, 48, 48, 1), (1, 2, 6, 80, 80, 1), (1, 2, 1, 56, 56, 1), (1, 2, 2, 56, 56, 1),
    (1, 3, 8, 64, 40, 1), (1, 2, 4, 56, 56, 1), (1, 2, 5, 56, 56, 1), (1, 2, 9, 32, 32, 1),
    (1, 2, 3, 156, 156, 2), (1, 2, 3, 78, 78, 1), (1, 2, 3, 78, 78, 2), (1, 2, 3, 39, 39, 1),   # X3D-L / XL planes (16 x 312 x 312 clips)
    (1, 2, 3, 20, 20, 2), (1, 2, 3, 10, 10, 1), (1, 2, 3, 80, 80, 2), (1, 2, 3, 40, 40, 1), (1, 2, 3, 40, 40, 2),  # + X3D-S planes
    (1, 2, 3, 10, 10, 2), (1, 2, 3, 5, 5, 1),
    (6, 3, 5, 14, 14, 1), (11, 2, 4, 10, 10, 1), (3, 2, 7, 12, 12, 1),   # packed backward (dw_pk.hip): one plane per wave, strips of 4 / 2
    (9, 3, 5, 7, 7, 1),                                                   #   7x7: four planes per wave (4 + 4 + 1), strips 4 + 3
    (3, 4, 8, 14, 14, 1), (2, 3, 1, 14, 14, 1), (2, 2, 2, 14, 14, 1),     # matrix-core kernels (dw_mx.hip, 16-bit storage): T % 4 == 0 runs the
    (2, 3, 13, 14, 14, 1),                                                #   exit-free loop (ring of 4), else ring of 3; T below the prefetch depth
    (5, 3, 4, 7, 7, 1), (2, 2, 8, 7, 7, 1), (4, 2, 16, 7, 7, 1),          #   7x7 planes four to a tile (partial last group), T % 4 == 0
    (2, 2, 4, 12, 14, 1), (1, 2, 5, 14, 12, 1),                           #   12 / 14 rows and columns
    (2, 3, 5, 28, 28, 1), (1, 2, 4, 26, 30, 1), (2, 2, 8, 28, 26, 1),     #   H-tiled backward for rows of 26 .. 30 elements (dw3d_bwd_mxw_kernel)
    # H- and W-tiled matrix-core backward for ragged rows (dw3d_bwd_mxg_kernel<bf16, NT, W-tiled, odd, ...>): one window of 3 column
    # tiles (39, 45, 44), two / three W-tiles (78 = 40 + 38, 91 = 32 + 32 + 27 odd), windows of 2 column tiles (30, 29, 54 = 28 + 26,
    # 55 = 28 + 27), both T loops, a partial last H-tile
    (2, 3, 4, 39, 39, 1), (1, 2, 8, 78, 78, 1), (1, 2, 5, 39, 39, 1), (1, 2, 4, 36, 45, 1), (1, 2, 4, 36, 44, 1), (1, 2, 4, 28, 91, 1),
    (1, 2, 4, 22, 30, 1), (1, 2, 4, 28, 29, 1), (2, 2, 4, 28, 54, 1), (1, 2, 5, 28, 55, 1), (1, 2, 7, 22, 78, 1),
    # ragged rows (flat staging, CV < 0): X3D-S 182-pixel test crops (91 / 46 / 23), vectors that cross rows and H-tiles,
    # rows shorter than a 16-byte vector (13 -> 7: 8-byte vectors), short planes
    (1, 2, 3, 91, 91, 1), (1, 2, 3, 91, 91, 2), (1, 2, 4, 46, 46, 1), (1, 2, 3, 23, 23, 1), (1, 2, 3, 23, 23, 2),
    (2, 2, 3, 13, 13, 2), (1, 2, 3, 6, 21, 1), (1, 1, 3, 30, 11, 1), (1, 2, 2, 3, 37, 1),
]

# ---- every depthwise launch of the full-size plans of BASELINE configs 2 - 5 (and config 3 with fp16 storage), for the fp64
# checks of tests/test_full_size_gpu.py.  Keyed by shape and launch form, not by kernel: after a rewrite the same case runs
# whatever the dispatch picks.  tests/test_dispatch_coverage.py asserts that every x3d_dw3d_fwd / x3d_dw3d_bwd launch of
# those dry plans has its entry here.
#   entry, dtype, N, C, T, H, W, stride, prologue, stats, pool
# prologue: "ss" (BN_a as a scale / shift table) or "bn" (its finalize folded into the launch, ops.bn_fold); stats: the BN_b
# sums are written (training); pool: the SE squeeze sums are written.  The stride-1 layers of every stage launch with and
# without pool (SE on every second block): one case with pool stands for both where the coverage test finds that the two
# dispatch the same kernel.  Backward launches have no form of their own (None, None, None).
def _dw_full(dtype, n, t, chans, s, pools, training):
    """The launches of one plan, stage by stage: the first block's stride-2 layer (with the SE pool where `pools` says so),
    then the stride-1 layer of the other blocks (pool on and off)."""
    out = []
    for i, (c, pool2) in enumerate(zip(chans, pools)):
        h = -(-s // 2 ** (i + 1))            # the stage's input extent (the stem halves S)
        for stride, hh, pool in ((2, h, pool2), (1, -(-h // 2), True)):
            out.append(("fwd", dtype, n, c, t, hh, hh, stride, "ss", training, pool))
            if training:
                out.append(("bwd", dtype, n, c, t, hh, hh, stride, None, None, None))
    return out


_W, _SM, _SL = (54, 108, 216, 432), (True, False, True, False), (True, False, False, True)
DW_FULL = (_dw_full(F32, 32, 13, _W, 160, _SM, True)                                   # config 2: X3D-S, fp32
           + _dw_full(BF16, 64, 16, _W, 224, _SM, True)                                # config 3: X3D-M (bench.py's workload)
           + _dw_full(F16, 64, 16, _W, 224, _SM, True)                                 # ... with fp16 storage (bench.py --dtype fp16)
           + _dw_full(BF16, 16, 16, _W, 312, _SL, True)                                # config 4: X3D-L
           + _dw_full(F16, 30, 16, (72, 162, 306, 630), 312, _SL, False))           # config 5: X3D-XL inference, 30 views


def dw_full_id(case):
    e, dt, n, c, t, h, w, s, pro, st, pool = case
    form = "" if e == "bwd" else f"-{pro}" + ("-stats" if st else "") + ("-pool" if pool else "")
    return f"{e}-{str(dt)[6:]}-N{n}-C{c}-T{t}-{h}x{w}-s{s}{form}"


# ---- every pointwise launch (x3d_pw_fwd / _dgrad / _wgrad / _bwd) of the same full-size plans, for the fp64 checks of
# tests/test_full_size_gpu.py; tests/test_dispatch_coverage.py keeps it complete and free of stale entries.  Keyed by shape
# and launch form, read from the argument struct, not by kernel.
#   entry, dtype, N, Cin, Cout, T, H, W, stride, epi, in_act, out_act, form
# H, W: the input extents of fwd / wgrad and of a bwd launch with x_stride = 2 (the strided recomputed-output shortcut),
# else the output points.  stride: fwd / wgrad stride, bwd x_stride (0 dense, 2 strided), None for dgrad.  epi: X3D_EPI_* of
# dgrad / bwd.  in_act: fwd / wgrad prologue activation; out_act: fwd.  form, in PW_FLAGS order:
#   fwd: stats; prologue ss (in_scale_shift) / gate (in_gate); tail fold add (in_add) / add_ss / store (in_store); inference
#        epilogue oss (out_scale_shift) / oadd (out_add) / oadd_ss (out_add_scale_shift)
#   dgrad / bwd: gate (SE gate of EPI_SWISH_BWD); tail_c / tail_r (folded residual-tail backward); rc (rc_panel: recomputed
#        conv output); slab (dw_slab); fold (coef_fold); pub (the fold publishes dgamma / dbeta / coef_out)
#   wgrad: ss / gate (prologue replayed); slab; fold
# A case with gate or pub stands for the launch of its shape without them only where the coverage test finds that both
# dispatch the same kernel instantiation (never the reverse).  16-bit fwd / dgrad / bwd launches pass the weight panel, as
# the plans do (rc launches need none).
PW_FLAGS = ("stats", "ss", "gate", "add", "add_ss", "store", "oss", "oadd", "oadd_ss", "tail_c", "tail_r", "rc", "slab", "fold",
            "pub")
PW_FULL = [
    # config 2: X3D-S, fp32
    ('fwd', F32, 32, 24, 54, 13, 80, 80, 1, None, 1, 0, ('stats', 'ss', 'store')),
    ('fwd', F32, 32, 54, 24, 13, 40, 40, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F32, 32, 24, 24, 13, 80, 80, 2, None, 0, 0, ('stats',)),
    ('fwd', F32, 32, 24, 54, 13, 40, 40, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F32, 32, 24, 54, 13, 40, 40, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F32, 32, 24, 108, 13, 40, 40, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F32, 32, 108, 48, 13, 20, 20, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F32, 32, 24, 48, 13, 40, 40, 2, None, 0, 0, ('stats',)),
    ('fwd', F32, 32, 48, 108, 13, 20, 20, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F32, 32, 48, 108, 13, 20, 20, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F32, 32, 48, 216, 13, 20, 20, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F32, 32, 216, 96, 13, 10, 10, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F32, 32, 48, 96, 13, 20, 20, 2, None, 0, 0, ('stats',)),
    ('fwd', F32, 32, 96, 216, 13, 10, 10, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F32, 32, 96, 216, 13, 10, 10, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F32, 32, 96, 432, 13, 10, 10, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F32, 32, 432, 192, 13, 5, 5, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F32, 32, 96, 192, 13, 5, 5, 1, None, 0, 0, ('stats',)),
    ('fwd', F32, 32, 192, 432, 13, 5, 5, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F32, 32, 192, 432, 13, 5, 5, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('wgrad', F32, 32, 192, 432, 13, 5, 5, 1, None, 0, None, ('fold',)),
    ('dgrad', F32, 32, 192, 432, 13, 5, 5, None, 0, None, None, ('fold', 'pub')),
    ('wgrad', F32, 32, 432, 192, 13, 5, 5, 1, None, 2, None, ('ss', 'gate', 'slab', 'fold')),
    ('dgrad', F32, 32, 432, 192, 13, 5, 5, None, 3, None, None, ('gate', 'fold', 'pub')),
    ('wgrad', F32, 32, 192, 432, 13, 5, 5, 1, None, 0, None, ('slab', 'fold')),
    ('dgrad', F32, 32, 192, 432, 13, 5, 5, None, 1, None, None, ('fold', 'pub')),
    ('wgrad', F32, 32, 96, 192, 13, 5, 5, 1, None, 0, None, ('fold',)),
    ('dgrad', F32, 32, 96, 192, 13, 5, 5, None, 0, None, None, ('fold', 'pub')),
    ('wgrad', F32, 32, 96, 432, 13, 10, 10, 1, None, 0, None, ()),
    ('dgrad', F32, 32, 96, 432, 13, 10, 10, None, 2, None, None, ()),
    ('wgrad', F32, 32, 216, 96, 13, 10, 10, 1, None, 2, None, ('ss', 'gate', 'slab', 'fold')),
    ('dgrad', F32, 32, 216, 96, 13, 10, 10, None, 3, None, None, ('gate', 'fold', 'pub')),
    ('wgrad', F32, 32, 96, 216, 13, 10, 10, 1, None, 0, None, ('slab', 'fold')),
    ('dgrad', F32, 32, 96, 216, 13, 10, 10, None, 1, None, None, ('fold', 'pub')),
    ('wgrad', F32, 32, 48, 96, 13, 20, 20, 2, None, 0, None, ()),
    ('dgrad', F32, 32, 48, 96, 13, 10, 10, None, 0, None, None, ()),
    ('wgrad', F32, 32, 48, 216, 13, 20, 20, 1, None, 0, None, ()),
    ('dgrad', F32, 32, 48, 216, 13, 20, 20, None, 2, None, None, ()),
    ('wgrad', F32, 32, 108, 48, 13, 20, 20, 1, None, 2, None, ('ss', 'gate', 'fold')),
    ('dgrad', F32, 32, 108, 48, 13, 20, 20, None, 3, None, None, ('gate', 'fold', 'pub')),
    ('wgrad', F32, 32, 48, 108, 13, 20, 20, 1, None, 0, None, ('fold',)),
    ('dgrad', F32, 32, 48, 108, 13, 20, 20, None, 1, None, None, ('fold', 'pub')),
    ('wgrad', F32, 32, 24, 48, 13, 40, 40, 2, None, 0, None, ()),
    ('dgrad', F32, 32, 24, 48, 13, 20, 20, None, 0, None, None, ()),
    ('wgrad', F32, 32, 24, 108, 13, 40, 40, 1, None, 0, None, ()),
    ('dgrad', F32, 32, 24, 108, 13, 40, 40, None, 2, None, None, ()),
    ('wgrad', F32, 32, 54, 24, 13, 40, 40, 1, None, 2, None, ('ss', 'gate', 'fold')),
    ('dgrad', F32, 32, 54, 24, 13, 40, 40, None, 3, None, None, ('gate', 'fold', 'pub')),
    ('wgrad', F32, 32, 24, 54, 13, 40, 40, 1, None, 0, None, ('fold',)),
    ('dgrad', F32, 32, 24, 54, 13, 40, 40, None, 1, None, None, ('fold', 'pub')),
    ('wgrad', F32, 32, 24, 24, 13, 80, 80, 2, None, 0, None, ()),
    ('dgrad', F32, 32, 24, 24, 13, 40, 40, None, 0, None, None, ()),
    ('wgrad', F32, 32, 24, 54, 13, 80, 80, 1, None, 0, None, ()),
    ('dgrad', F32, 32, 24, 54, 13, 80, 80, None, 2, None, None, ()),
    # config 3: X3D-M (bench.py's workload)
    ('fwd', BF16, 64, 24, 54, 16, 112, 112, 1, None, 1, 0, ('stats', 'ss', 'store')),
    ('fwd', BF16, 64, 54, 24, 16, 56, 56, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 64, 24, 24, 16, 112, 112, 2, None, 0, 0, ('stats',)),
    ('fwd', BF16, 64, 24, 54, 16, 56, 56, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 64, 24, 54, 16, 56, 56, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 64, 24, 108, 16, 56, 56, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 64, 108, 48, 16, 28, 28, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 64, 24, 48, 16, 56, 56, 2, None, 0, 0, ('stats',)),
    ('fwd', BF16, 64, 48, 108, 16, 28, 28, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 64, 48, 108, 16, 28, 28, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 64, 48, 216, 16, 28, 28, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 64, 216, 96, 16, 14, 14, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 64, 48, 96, 16, 28, 28, 2, None, 0, 0, ('stats',)),
    ('fwd', BF16, 64, 96, 216, 16, 14, 14, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 64, 96, 216, 16, 14, 14, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 64, 96, 432, 16, 14, 14, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 64, 432, 192, 16, 7, 7, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 64, 96, 192, 16, 7, 7, 1, None, 0, 0, ('stats',)),
    ('fwd', BF16, 64, 192, 432, 16, 7, 7, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 64, 192, 432, 16, 7, 7, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('wgrad', BF16, 64, 192, 432, 16, 7, 7, 1, None, 0, None, ('fold',)),
    ('dgrad', BF16, 64, 192, 432, 16, 7, 7, None, 0, None, None, ('fold', 'pub')),
    ('bwd', BF16, 64, 432, 192, 16, 7, 7, 0, 3, None, None, ('gate', 'slab', 'fold', 'pub')),
    ('wgrad', BF16, 64, 192, 432, 16, 7, 7, 1, None, 0, None, ('slab', 'fold')),
    ('dgrad', BF16, 64, 192, 432, 16, 7, 7, None, 1, None, None, ('fold', 'pub')),
    ('wgrad', BF16, 64, 96, 192, 16, 7, 7, 1, None, 0, None, ('fold',)),
    ('dgrad', BF16, 64, 96, 192, 16, 7, 7, None, 0, None, None, ('fold', 'pub')),
    ('wgrad', BF16, 64, 96, 432, 16, 14, 14, 1, None, 0, None, ('fold',)),
    ('dgrad', BF16, 64, 96, 432, 16, 14, 14, None, 2, None, None, ('fold', 'pub')),
    ('bwd', BF16, 64, 216, 96, 16, 14, 14, 0, 3, None, None, ('gate', 'slab', 'fold', 'pub')),
    ('bwd', BF16, 64, 96, 216, 16, 14, 14, 0, 1, None, None, ('tail_c', 'slab', 'fold', 'pub')),
    ('bwd', BF16, 64, 96, 216, 16, 14, 14, 0, 1, None, None, ('slab', 'fold', 'pub')),
    ('bwd', BF16, 64, 48, 96, 16, 28, 28, 2, 0, None, None, ('rc',)),
    ('bwd', BF16, 64, 48, 216, 16, 28, 28, 0, 2, None, None, ('rc',)),
    ('bwd', BF16, 64, 108, 48, 16, 28, 28, 0, 3, None, None, ('gate',)),
    ('bwd', BF16, 64, 48, 108, 16, 28, 28, 0, 1, None, None, ('rc',)),
    ('bwd', BF16, 64, 24, 48, 16, 56, 56, 2, 0, None, None, ('rc',)),
    ('bwd', BF16, 64, 24, 108, 16, 56, 56, 0, 2, None, None, ('tail_c', 'rc')),
    ('bwd', BF16, 64, 54, 24, 16, 56, 56, 0, 3, None, None, ('gate',)),
    ('bwd', BF16, 64, 24, 54, 16, 56, 56, 0, 1, None, None, ('tail_c', 'rc')),
    ('bwd', BF16, 64, 24, 54, 16, 56, 56, 0, 1, None, None, ('tail_c', 'tail_r', 'rc')),
    ('bwd', BF16, 64, 24, 24, 16, 112, 112, 2, 0, None, None, ('rc',)),
    ('bwd', BF16, 64, 24, 54, 16, 112, 112, 0, 2, None, None, ('tail_c', 'rc')),
    # config 3 with fp16 storage
    ('fwd', F16, 64, 24, 54, 16, 112, 112, 1, None, 1, 0, ('stats', 'ss', 'store')),
    ('fwd', F16, 64, 54, 24, 16, 56, 56, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F16, 64, 24, 24, 16, 112, 112, 2, None, 0, 0, ('stats',)),
    ('fwd', F16, 64, 24, 54, 16, 56, 56, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F16, 64, 24, 54, 16, 56, 56, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F16, 64, 24, 108, 16, 56, 56, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F16, 64, 108, 48, 16, 28, 28, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F16, 64, 24, 48, 16, 56, 56, 2, None, 0, 0, ('stats',)),
    ('fwd', F16, 64, 48, 108, 16, 28, 28, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F16, 64, 48, 108, 16, 28, 28, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F16, 64, 48, 216, 16, 28, 28, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F16, 64, 216, 96, 16, 14, 14, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F16, 64, 48, 96, 16, 28, 28, 2, None, 0, 0, ('stats',)),
    ('fwd', F16, 64, 96, 216, 16, 14, 14, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F16, 64, 96, 216, 16, 14, 14, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F16, 64, 96, 432, 16, 14, 14, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', F16, 64, 432, 192, 16, 7, 7, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', F16, 64, 96, 192, 16, 7, 7, 1, None, 0, 0, ('stats',)),
    ('fwd', F16, 64, 192, 432, 16, 7, 7, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', F16, 64, 192, 432, 16, 7, 7, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('wgrad', F16, 64, 192, 432, 16, 7, 7, 1, None, 0, None, ('fold',)),
    ('dgrad', F16, 64, 192, 432, 16, 7, 7, None, 0, None, None, ('fold', 'pub')),
    ('bwd', F16, 64, 432, 192, 16, 7, 7, 0, 3, None, None, ('gate', 'slab', 'fold', 'pub')),
    ('wgrad', F16, 64, 192, 432, 16, 7, 7, 1, None, 0, None, ('slab', 'fold')),
    ('dgrad', F16, 64, 192, 432, 16, 7, 7, None, 1, None, None, ('fold', 'pub')),
    ('wgrad', F16, 64, 96, 192, 16, 7, 7, 1, None, 0, None, ('fold',)),
    ('dgrad', F16, 64, 96, 192, 16, 7, 7, None, 0, None, None, ('fold', 'pub')),
    ('wgrad', F16, 64, 96, 432, 16, 14, 14, 1, None, 0, None, ('fold',)),
    ('dgrad', F16, 64, 96, 432, 16, 14, 14, None, 2, None, None, ('fold', 'pub')),
    ('bwd', F16, 64, 216, 96, 16, 14, 14, 0, 3, None, None, ('gate', 'slab', 'fold', 'pub')),
    ('bwd', F16, 64, 96, 216, 16, 14, 14, 0, 1, None, None, ('tail_c', 'slab', 'fold', 'pub')),
    ('bwd', F16, 64, 96, 216, 16, 14, 14, 0, 1, None, None, ('slab', 'fold', 'pub')),
    ('bwd', F16, 64, 48, 96, 16, 28, 28, 2, 0, None, None, ('rc',)),
    ('bwd', F16, 64, 48, 216, 16, 28, 28, 0, 2, None, None, ('rc',)),
    ('bwd', F16, 64, 108, 48, 16, 28, 28, 0, 3, None, None, ('gate',)),
    ('bwd', F16, 64, 48, 108, 16, 28, 28, 0, 1, None, None, ('rc',)),
    ('bwd', F16, 64, 24, 48, 16, 56, 56, 2, 0, None, None, ('rc',)),
    ('bwd', F16, 64, 24, 108, 16, 56, 56, 0, 2, None, None, ('tail_c', 'rc')),
    ('bwd', F16, 64, 54, 24, 16, 56, 56, 0, 3, None, None, ('gate',)),
    ('bwd', F16, 64, 24, 54, 16, 56, 56, 0, 1, None, None, ('tail_c', 'rc')),
    ('bwd', F16, 64, 24, 54, 16, 56, 56, 0, 1, None, None, ('tail_c', 'tail_r', 'rc')),
    ('bwd', F16, 64, 24, 24, 16, 112, 112, 2, 0, None, None, ('rc',)),
    ('bwd', F16, 64, 24, 54, 16, 112, 112, 0, 2, None, None, ('tail_c', 'rc')),
    # config 4: X3D-L
    ('fwd', BF16, 16, 24, 54, 16, 156, 156, 1, None, 1, 0, ('stats', 'ss', 'store')),
    ('fwd', BF16, 16, 54, 24, 16, 78, 78, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 16, 24, 24, 16, 156, 156, 2, None, 0, 0, ('stats',)),
    ('fwd', BF16, 16, 24, 54, 16, 78, 78, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 16, 24, 54, 16, 78, 78, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 16, 24, 108, 16, 78, 78, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 16, 108, 48, 16, 39, 39, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 16, 24, 48, 16, 39, 39, 1, None, 0, 0, ('stats',)),
    ('fwd', BF16, 16, 48, 108, 16, 39, 39, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 16, 48, 108, 16, 39, 39, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 16, 48, 216, 16, 39, 39, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 16, 216, 96, 16, 20, 20, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 16, 48, 96, 16, 39, 39, 2, None, 0, 0, ('stats',)),
    ('fwd', BF16, 16, 96, 216, 16, 20, 20, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 16, 96, 216, 16, 20, 20, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 16, 96, 432, 16, 20, 20, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('fwd', BF16, 16, 432, 192, 16, 10, 10, 1, None, 2, 0, ('stats', 'ss', 'gate')),
    ('fwd', BF16, 16, 96, 192, 16, 20, 20, 2, None, 0, 0, ('stats',)),
    ('fwd', BF16, 16, 192, 432, 16, 10, 10, 1, None, 1, 0, ('stats', 'ss', 'add', 'add_ss', 'store')),
    ('fwd', BF16, 16, 192, 432, 16, 10, 10, 1, None, 1, 0, ('stats', 'ss', 'add', 'store')),
    ('wgrad', BF16, 16, 192, 432, 16, 10, 10, 1, None, 0, None, ('fold',)),
    ('dgrad', BF16, 16, 192, 432, 16, 10, 10, None, 0, None, None, ('fold', 'pub')),
    ('bwd', BF16, 16, 432, 192, 16, 10, 10, 0, 3, None, None, ('gate', 'slab', 'fold', 'pub')),
    ('wgrad', BF16, 16, 192, 432, 16, 10, 10, 1, None, 0, None, ('slab', 'fold')),
    ('dgrad', BF16, 16, 192, 432, 16, 10, 10, None, 1, None, None, ('fold', 'pub')),
    ('wgrad', BF16, 16, 96, 192, 16, 20, 20, 2, None, 0, None, ('fold',)),
    ('dgrad', BF16, 16, 96, 192, 16, 10, 10, None, 0, None, None, ('fold', 'pub')),
    ('wgrad', BF16, 16, 96, 432, 16, 20, 20, 1, None, 0, None, ('fold',)),
    ('dgrad', BF16, 16, 96, 432, 16, 20, 20, None, 2, None, None, ('fold', 'pub')),
    ('bwd', BF16, 16, 216, 96, 16, 20, 20, 0, 3, None, None, ('gate', 'slab', 'fold', 'pub')),
    ('bwd', BF16, 16, 96, 216, 16, 20, 20, 0, 1, None, None, ('tail_c', 'slab', 'fold', 'pub')),
    ('bwd', BF16, 16, 96, 216, 16, 20, 20, 0, 1, None, None, ('slab', 'fold', 'pub')),
    ('bwd', BF16, 16, 48, 96, 16, 39, 39, 2, 0, None, None, ('rc',)),
    ('bwd', BF16, 16, 48, 216, 16, 39, 39, 0, 2, None, None, ('rc',)),
    ('bwd', BF16, 16, 108, 48, 16, 39, 39, 0, 3, None, None, ('gate',)),
    ('bwd', BF16, 16, 48, 108, 16, 39, 39, 0, 1, None, None, ('rc',)),
    ('bwd', BF16, 16, 24, 48, 16, 39, 39, 0, 0, None, None, ('rc',)),
    ('bwd', BF16, 16, 24, 108, 16, 78, 78, 0, 2, None, None, ('tail_c', 'rc')),
    ('bwd', BF16, 16, 54, 24, 16, 78, 78, 0, 3, None, None, ('gate',)),
    ('bwd', BF16, 16, 24, 54, 16, 78, 78, 0, 1, None, None, ('tail_c', 'rc')),
    ('bwd', BF16, 16, 24, 54, 16, 78, 78, 0, 1, None, None, ('tail_c', 'tail_r', 'rc')),
    ('bwd', BF16, 16, 24, 24, 16, 156, 156, 2, 0, None, None, ('rc',)),
    ('bwd', BF16, 16, 24, 54, 16, 156, 156, 0, 2, None, None, ('tail_c', 'rc')),
    # config 5: X3D-XL inference, 30 views
    ('fwd', F16, 30, 32, 72, 16, 156, 156, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 32, 32, 16, 156, 156, 2, None, 0, 0, ()),
    ('fwd', F16, 30, 72, 32, 16, 78, 78, 1, None, 2, 1, ('ss', 'gate', 'oss', 'oadd', 'oadd_ss')),
    ('fwd', F16, 30, 32, 72, 16, 78, 78, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 72, 32, 16, 78, 78, 1, None, 2, 1, ('ss', 'gate', 'oss', 'oadd')),
    ('fwd', F16, 30, 32, 162, 16, 78, 78, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 32, 72, 16, 39, 39, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 162, 72, 16, 39, 39, 1, None, 2, 1, ('ss', 'oss', 'oadd', 'oadd_ss')),
    ('fwd', F16, 30, 72, 162, 16, 39, 39, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 162, 72, 16, 39, 39, 1, None, 2, 1, ('ss', 'gate', 'oss', 'oadd')),
    ('fwd', F16, 30, 72, 306, 16, 39, 39, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 72, 136, 16, 39, 39, 2, None, 0, 0, ()),
    ('fwd', F16, 30, 306, 136, 16, 20, 20, 1, None, 2, 1, ('ss', 'oss', 'oadd', 'oadd_ss')),
    ('fwd', F16, 30, 136, 306, 16, 20, 20, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 306, 136, 16, 20, 20, 1, None, 2, 1, ('ss', 'gate', 'oss', 'oadd')),
    ('fwd', F16, 30, 136, 630, 16, 20, 20, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 136, 280, 16, 20, 20, 2, None, 0, 0, ()),
    ('fwd', F16, 30, 630, 280, 16, 10, 10, 1, None, 2, 1, ('ss', 'gate', 'oss', 'oadd', 'oadd_ss')),
    ('fwd', F16, 30, 280, 630, 16, 10, 10, 1, None, 0, 0, ()),
    ('fwd', F16, 30, 630, 280, 16, 10, 10, 1, None, 2, 1, ('ss', 'gate', 'oss', 'oadd')),
]


def pw_full_id(case):
    e, dt, n, ci, co, t, h, w, s, epi, ia, oa, form = case
    mode = ("" if s is None else f"-s{s}") + ("" if epi is None else f"-e{epi}") + ("" if ia is None else f"-a{ia}") + \
        (f"-o{oa}" if oa else "")
    return f"{e}-{str(dt)[6:]}-N{n}-{ci}to{co}-T{t}-{h}x{w}{mode}" + "".join(f"-{f}" for f in form)


def pw_full_struct(case):
    """The argument struct of a PW_FULL case over address-only operands, in the case's launch form (a fold is a real
    hip.BnBwdFold the struct refers to by address; slabs are sized by the library's own dw_parts query)."""
    import ctypes as C
    from x3d_tf_amd import hip
    e, dtype, n, ci, co, t, h, w, s, epi, ia, oa, form = case
    A = _Addr.new
    f = set(form)
    opt = lambda k: A() if k in f else None
    panel = A() if dtype != F32 else None
    code = _code(dtype)
    if e == "fwd":
        return hip.PwFwdArgs(A(), A(), A(), opt("stats"), opt("ss"), opt("gate"), ia, n, ci, co, t, h, w, s, code, panel,
                             in_add=opt("add"), in_add_scale_shift=opt("add_ss"), in_store=opt("store"),
                             out_scale_shift=opt("oss"), out_add=opt("oadd"), out_add_scale_shift=opt("oadd_ss"), out_act=oa)
    if e == "dgrad":
        sw = epi == 3
        a = hip.PwDgradArgs(A(), A(), A(), A(), A(), epi, A() if epi in (1, 2) else None, A() if sw else None,
                            A() if sw else None, opt("gate"), A() if sw else None, n, ci, co, t, h, w, code, panel)
        query = None
    elif e == "wgrad":
        a = hip.PwWgradArgs(A(), A(), A(), A(), opt("ss"), opt("gate"), ia, A(), n, ci, co, t, h, w, s, code)
        query = hip.load().x3d_pw_wgrad_dw_parts
    elif "rc" in f:
        ho, wo = (-(-h // 2), -(-w // 2)) if s == 2 else (h, w)
        a = hip.PwBwdArgs(A(), None, None, None, A(), epi, A() if epi in (1, 2) else None, None, None, None, None, A(), None, n,
                          ci, co, t, ho, wo, code, opt("tail_c"), opt("tail_r"), opt("tail_c"), opt("tail_r"), A(), A(), A(),
                          s, h, w)
        query = None
    else:
        sw = epi == 3
        a = hip.PwBwdArgs(A(), A(), A(), panel, A(), epi, None if sw else A(), A() if sw else None, A() if sw else None,
                          opt("gate"), A() if sw else None, None if sw else A(), A(), n, ci, co, t, h, w, code, opt("tail_c"),
                          opt("tail_r"), opt("tail_c"), opt("tail_r"))
        query = hip.load().x3d_pw_bwd_dw_parts
    if "fold" in f:
        a._fold = hip.BnBwdFold(A(), 1.0, A(), A(), A() if "pub" in f else None, A() if "pub" in f else None,
                                A() if "pub" in f else None)
        a.coef_fold = hip.fold_address(a._fold)
    if "slab" in f:
        a.dw_slab_parts = int(query(C.byref(a)))
        a.dw_slab = A()
    return a


# ---- every other launch of the same plans (tests/test_full_size_gpu.py: test_aux_full_size; tests/test_dispatch_coverage.py
# keeps the list complete): BatchNorm bookkeeping, the residual tail's backward, squeeze-excite with the slab reductions it
# carries, the head, the loss.  One key per launch form, read from the recorded arguments (C ABI order; the struct for
# x3d_se_bnb_bwd), with every argument that picks an instantiation (the dtype, P -- VEC and the small-plane tail_bwd -- and
# the null / non-null optional pointers):
#   ("tail_bwd", dtype, N, C, P, has_r)                   ("relu_bn_bwd_reduce", dtype, N, C, P, "dy" | "dpool", g_written)
#   ("pool_fwd", dtype, N, C, P)                          ("subsample2", dtype, planes, H, W)
#   ("se_fwd", N, C, Wd, P)                               ("se_bnb_bwd", N, C, Wd, P, has_se, ((slab parts, elems), ...))
#   ("dense_fwd", N, K, M, act, mask_scale | None, bias)  ("dense_bwd", N, K, M, act, mask_scale | None, dx, db)
#   ("softmax_xent", N, M, grad_scale, training)          ("view_mean", videos, views, M)
#   ("bn_finalize", C, count, update_moving)              ("bn_bwd_finalize", C, count)
#   ("bn_bwd_finalize_rc", dtype, C, count, prepare Cin | 0, (finish Cout, Cin) | None)
#   ("bn_eval_coef_batched", channels of every table item)
_XL_BN = (32, 72, 72, 32, 32, 72, 72, 32, 72, 72, 32, 72, 72, 32, 72, 72, 32, 162, 162, 72, 72, 162, 162, 72, 162, 162, 72, 162,
           162, 72, 162, 162, 72, 162, 162, 72, 162, 162, 72, 162, 162, 72, 162, 162, 72, 162, 162, 72, 306, 306, 136, 136, 306,
           306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136,
           306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306,
           136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306, 306, 136, 306,
           306, 136, 630, 630, 280, 280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630, 630,
           280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630, 630, 280, 630,
           630, 280, 630)
AUX_FULL = [
    # bn_finalize
    ("bn_finalize", 24, 2662400, 1), ("bn_finalize", 54, 2662400, 1), ("bn_finalize", 54, 665600, 1),
    ("bn_finalize", 24, 665600, 1), ("bn_finalize", 108, 665600, 1), ("bn_finalize", 108, 166400, 1),
    ("bn_finalize", 48, 166400, 1), ("bn_finalize", 216, 166400, 1), ("bn_finalize", 216, 41600, 1),
    ("bn_finalize", 96, 41600, 1), ("bn_finalize", 432, 41600, 1), ("bn_finalize", 432, 10400, 1),
    ("bn_finalize", 192, 10400, 1), ("bn_finalize", 24, 12845056, 1), ("bn_finalize", 54, 12845056, 1),
    ("bn_finalize", 54, 3211264, 1), ("bn_finalize", 24, 3211264, 1), ("bn_finalize", 108, 3211264, 1),
    ("bn_finalize", 108, 802816, 1), ("bn_finalize", 48, 802816, 1), ("bn_finalize", 216, 802816, 1),
    ("bn_finalize", 216, 200704, 1), ("bn_finalize", 96, 200704, 1), ("bn_finalize", 432, 200704, 1),
    ("bn_finalize", 432, 50176, 1), ("bn_finalize", 192, 50176, 1), ("bn_finalize", 24, 6230016, 1),
    ("bn_finalize", 54, 6230016, 1), ("bn_finalize", 54, 1557504, 1), ("bn_finalize", 24, 1557504, 1),
    ("bn_finalize", 108, 1557504, 1), ("bn_finalize", 108, 389376, 1), ("bn_finalize", 48, 389376, 1),
    ("bn_finalize", 216, 389376, 1), ("bn_finalize", 216, 102400, 1), ("bn_finalize", 96, 102400, 1),
    ("bn_finalize", 432, 102400, 1), ("bn_finalize", 432, 25600, 1), ("bn_finalize", 192, 25600, 1),
    # se_fwd
    ("se_fwd", 32, 54, 8, 20800), ("se_fwd", 32, 108, 8, 5200), ("se_fwd", 32, 216, 16, 1300), ("se_fwd", 32, 432, 32, 325),
    ("se_fwd", 64, 54, 8, 50176), ("se_fwd", 64, 108, 8, 12544), ("se_fwd", 64, 216, 16, 3136), ("se_fwd", 64, 432, 32, 784),
    ("se_fwd", 16, 54, 8, 97344), ("se_fwd", 16, 108, 8, 24336), ("se_fwd", 16, 216, 16, 6400), ("se_fwd", 16, 432, 32, 1600),
    ("se_fwd", 30, 72, 8, 97344), ("se_fwd", 30, 162, 16, 24336), ("se_fwd", 30, 306, 24, 6400), ("se_fwd", 30, 630, 40, 1600),
    # subsample2
    ("subsample2", F32, 39936, 10, 10), ("subsample2", BF16, 98304, 14, 14), ("subsample2", F16, 98304, 14, 14),
    ("subsample2", BF16, 6144, 78, 78), ("subsample2", F16, 15360, 78, 78),
    # pool_fwd
    ("pool_fwd", F32, 32, 432, 325), ("pool_fwd", BF16, 64, 432, 784), ("pool_fwd", F16, 64, 432, 784),
    ("pool_fwd", BF16, 16, 432, 1600), ("pool_fwd", F16, 30, 630, 1600),
    # dense_fwd
    ("dense_fwd", 32, 432, 2048, 1, None, False), ("dense_fwd", 32, 2048, 400, 0, 2.0, True),
    ("dense_fwd", 64, 432, 2048, 1, None, False), ("dense_fwd", 64, 2048, 400, 0, 2.0, True),
    ("dense_fwd", 16, 432, 2048, 1, None, False), ("dense_fwd", 16, 2048, 400, 0, 2.0, True),
    ("dense_fwd", 30, 630, 2048, 1, None, False), ("dense_fwd", 30, 2048, 400, 0, None, True),
    # softmax_xent
    ("softmax_xent", 32, 400, 0.03125, True), ("softmax_xent", 64, 400, 0.015625, True),
    ("softmax_xent", 16, 400, 0.0625, True), ("softmax_xent", 30, 400, 1.0, False),
    # dense_bwd
    ("dense_bwd", 32, 2048, 400, 0, 2.0, True, True), ("dense_bwd", 32, 432, 2048, 1, None, True, False),
    ("dense_bwd", 64, 2048, 400, 0, 2.0, True, True), ("dense_bwd", 64, 432, 2048, 1, None, True, False),
    ("dense_bwd", 16, 2048, 400, 0, 2.0, True, True), ("dense_bwd", 16, 432, 2048, 1, None, True, False),
    # relu_bn_bwd_reduce
    ("relu_bn_bwd_reduce", F32, 32, 432, 325, "dpool", True), ("relu_bn_bwd_reduce", F32, 32, 24, 83200, "dy", False),
    ("relu_bn_bwd_reduce", BF16, 64, 432, 784, "dpool", True), ("relu_bn_bwd_reduce", F16, 64, 432, 784, "dpool", True),
    ("relu_bn_bwd_reduce", BF16, 16, 432, 1600, "dpool", True),
    # tail_bwd
    ("tail_bwd", F32, 32, 192, 325, False), ("tail_bwd", F32, 32, 192, 325, True), ("tail_bwd", F32, 32, 96, 1300, False),
    ("tail_bwd", F32, 32, 96, 1300, True), ("tail_bwd", F32, 32, 48, 5200, False), ("tail_bwd", F32, 32, 48, 5200, True),
    ("tail_bwd", F32, 32, 24, 20800, False), ("tail_bwd", F32, 32, 24, 20800, True), ("tail_bwd", BF16, 64, 192, 784, False),
    ("tail_bwd", BF16, 64, 192, 784, True), ("tail_bwd", BF16, 64, 96, 3136, False), ("tail_bwd", BF16, 64, 96, 3136, True),
    ("tail_bwd", BF16, 64, 48, 12544, False), ("tail_bwd", BF16, 64, 48, 12544, True), ("tail_bwd", F16, 64, 192, 784, False),
    ("tail_bwd", F16, 64, 192, 784, True), ("tail_bwd", F16, 64, 96, 3136, False), ("tail_bwd", F16, 64, 96, 3136, True),
    ("tail_bwd", F16, 64, 48, 12544, False), ("tail_bwd", F16, 64, 48, 12544, True), ("tail_bwd", BF16, 16, 192, 1600, False),
    ("tail_bwd", BF16, 16, 192, 1600, True), ("tail_bwd", BF16, 16, 96, 6400, False), ("tail_bwd", BF16, 16, 96, 6400, True),
    ("tail_bwd", BF16, 16, 48, 24336, False), ("tail_bwd", BF16, 16, 48, 24336, True),
    # se_bnb_bwd
    ("se_bnb_bwd", 32, 432, 0, 325, False, ((32, 82944),)), ("se_bnb_bwd", 32, 432, 32, 325, True, ((32, 82944), (32, 82944))),
    ("se_bnb_bwd", 32, 432, 0, 325, False, ((32, 82944), (32, 82944))),
    ("se_bnb_bwd", 32, 216, 16, 1300, True, ((128, 20736),)),
    ("se_bnb_bwd", 32, 216, 0, 1300, False, ((128, 20736), (128, 20736))),
    ("se_bnb_bwd", 32, 216, 16, 1300, True, ((128, 20736), (128, 20736))), ("se_bnb_bwd", 32, 108, 0, 5200, False, ()),
    ("se_bnb_bwd", 32, 108, 8, 5200, True, ()), ("se_bnb_bwd", 32, 54, 8, 20800, True, ()),
    ("se_bnb_bwd", 32, 54, 0, 20800, False, ()), ("se_bnb_bwd", 64, 432, 0, 784, False, ((124, 82944),)),
    ("se_bnb_bwd", 64, 432, 32, 784, True, ((124, 82944), (64, 82944))),
    ("se_bnb_bwd", 64, 432, 0, 784, False, ((124, 82944), (64, 82944))),
    ("se_bnb_bwd", 64, 216, 16, 3136, True, ((251, 20736),)),
    ("se_bnb_bwd", 64, 216, 0, 3136, False, ((251, 20736), (251, 20736))),
    ("se_bnb_bwd", 64, 216, 16, 3136, True, ((251, 20736), (251, 20736))), ("se_bnb_bwd", 64, 108, 0, 12544, False, ()),
    ("se_bnb_bwd", 64, 108, 8, 12544, True, ()), ("se_bnb_bwd", 64, 54, 8, 50176, True, ()),
    ("se_bnb_bwd", 64, 54, 0, 50176, False, ()), ("se_bnb_bwd", 16, 432, 32, 1600, True, ((115, 82944),)),
    ("se_bnb_bwd", 16, 432, 0, 1600, False, ((115, 82944), (56, 82944))),
    ("se_bnb_bwd", 16, 432, 32, 1600, True, ((115, 82944), (56, 82944))),
    ("se_bnb_bwd", 16, 216, 0, 6400, False, ((247, 20736),)),
    ("se_bnb_bwd", 16, 216, 16, 6400, True, ((247, 20736), (247, 20736))),
    ("se_bnb_bwd", 16, 216, 0, 6400, False, ((247, 20736), (247, 20736))), ("se_bnb_bwd", 16, 108, 8, 24336, True, ()),
    ("se_bnb_bwd", 16, 108, 0, 24336, False, ()), ("se_bnb_bwd", 16, 54, 8, 97344, True, ()),
    ("se_bnb_bwd", 16, 54, 0, 97344, False, ()),
    # bn_bwd_finalize
    ("bn_bwd_finalize", 432, 41600), ("bn_bwd_finalize", 96, 41600), ("bn_bwd_finalize", 216, 166400),
    ("bn_bwd_finalize", 48, 166400), ("bn_bwd_finalize", 108, 665600), ("bn_bwd_finalize", 24, 665600),
    ("bn_bwd_finalize", 54, 2662400), ("bn_bwd_finalize", 24, 2662400),
    # bn_bwd_finalize_rc
    ("bn_bwd_finalize_rc", BF16, 96, 200704, 48, None), ("bn_bwd_finalize_rc", BF16, 216, 802816, 48, (96, 48)),
    ("bn_bwd_finalize_rc", BF16, 48, 802816, 0, (216, 48)), ("bn_bwd_finalize_rc", BF16, 108, 802816, 48, None),
    ("bn_bwd_finalize_rc", BF16, 48, 802816, 0, (108, 48)), ("bn_bwd_finalize_rc", BF16, 48, 802816, 24, None),
    ("bn_bwd_finalize_rc", BF16, 108, 3211264, 24, (48, 24)), ("bn_bwd_finalize_rc", BF16, 24, 3211264, 0, (108, 24)),
    ("bn_bwd_finalize_rc", BF16, 54, 3211264, 24, None), ("bn_bwd_finalize_rc", BF16, 24, 3211264, 0, (54, 24)),
    ("bn_bwd_finalize_rc", BF16, 24, 3211264, 24, None), ("bn_bwd_finalize_rc", BF16, 54, 12845056, 24, (24, 24)),
    ("bn_bwd_finalize_rc", BF16, 24, 12845056, 0, (54, 24)), ("bn_bwd_finalize_rc", F16, 96, 200704, 48, None),
    ("bn_bwd_finalize_rc", F16, 216, 802816, 48, (96, 48)), ("bn_bwd_finalize_rc", F16, 48, 802816, 0, (216, 48)),
    ("bn_bwd_finalize_rc", F16, 108, 802816, 48, None), ("bn_bwd_finalize_rc", F16, 48, 802816, 0, (108, 48)),
    ("bn_bwd_finalize_rc", F16, 48, 802816, 24, None), ("bn_bwd_finalize_rc", F16, 108, 3211264, 24, (48, 24)),
    ("bn_bwd_finalize_rc", F16, 24, 3211264, 0, (108, 24)), ("bn_bwd_finalize_rc", F16, 54, 3211264, 24, None),
    ("bn_bwd_finalize_rc", F16, 24, 3211264, 0, (54, 24)), ("bn_bwd_finalize_rc", F16, 24, 3211264, 24, None),
    ("bn_bwd_finalize_rc", F16, 54, 12845056, 24, (24, 24)), ("bn_bwd_finalize_rc", F16, 24, 12845056, 0, (54, 24)),
    ("bn_bwd_finalize_rc", BF16, 96, 102400, 48, None), ("bn_bwd_finalize_rc", BF16, 216, 389376, 48, (96, 48)),
    ("bn_bwd_finalize_rc", BF16, 48, 389376, 0, (216, 48)), ("bn_bwd_finalize_rc", BF16, 108, 389376, 48, None),
    ("bn_bwd_finalize_rc", BF16, 48, 389376, 0, (108, 48)), ("bn_bwd_finalize_rc", BF16, 48, 389376, 24, None),
    ("bn_bwd_finalize_rc", BF16, 108, 1557504, 24, (48, 24)), ("bn_bwd_finalize_rc", BF16, 24, 1557504, 0, (108, 24)),
    ("bn_bwd_finalize_rc", BF16, 54, 1557504, 24, None), ("bn_bwd_finalize_rc", BF16, 24, 1557504, 0, (54, 24)),
    ("bn_bwd_finalize_rc", BF16, 24, 1557504, 24, None), ("bn_bwd_finalize_rc", BF16, 54, 6230016, 24, (24, 24)),
    ("bn_bwd_finalize_rc", BF16, 24, 6230016, 0, (54, 24)),
    # bn_eval_coef_batched: the whole X3D-XL inference BatchNorm table (config 5), channels of its 171 items in table order
    ("bn_eval_coef_batched", _XL_BN),
    # view_mean
    ("view_mean", 1, 30, 400),
]


def aux_full_id(case):
    e = case[0]
    if e == "bn_eval_coef_batched":
        return f"{e}-{len(case[1])}items"
    f = lambda v: str(v)[6:] if isinstance(v, torch.dtype) else ("x".join(map(str, v)) if isinstance(v, tuple) and v and
                                                                  isinstance(v[0], int) else str(v))
    parts = [f(v) if not (isinstance(v, tuple) and v and isinstance(v[0], tuple)) else "+".join(f(j) for j in v) or "nojobs"
             for v in case[1:]]
    return "-".join([e] + [p if p else "none" for p in parts])


# ---- the same runners (tests/aux_checks.py) at the edges of the kernels' tiles: tests/test_aux_edges_gpu.py runs every case,
# tests/test_aux_edges.py keeps the table on the edges when a tile size is retuned.  Keys as AUX_FULL, the plane-wise ones with an
# optional trailing element offset of every tensor into its allocation (a view that is not 16-byte aligned), and
#   ("tail_fwd", dtype, N, C, P, None | "identity" | "conv"[, off])      ("dw_slab_reduce", ((parts, elems), ...))
#   ("all_finite", n, kind, pos)     ("l2_sumsq", n, None | "random" | "zeros")     ("nthwc_to_ncthw", src, dst, N, C, P[, off])
#   ("dense_bwd_refused", N, K, M)   ("se_fwd_refused", N, C, Wd)                   ("dw_slab_reduce_refused", parts, elems, off)
# The tile sizes the table was built for: the #define lines of head.hip, se.hip and elem.hip (test_aux_edges.py reads them from the
# sources and fails when one moved), and the literals of the kernels' loops:
AUX_TILES = dict(DENSE_NT=8, DENSE_MT=4, DENSE_BN=4, DENSE_BM=8, SE_MAXC=1024, SE_MAXW=64, DWR_EPB=64, ELEM_BLOCK=256, ELEM_ITERS=4)
AUX_TILE_SOURCES = {"head.hip": ("DENSE_NT", "DENSE_MT", "DENSE_BN", "DENSE_BM"), "se.hip": ("SE_MAXC", "SE_MAXW", "DWR_EPB"),
                    "elem.hip": ("ELEM_BLOCK", "ELEM_ITERS")}
AUX_LITERALS = dict(
    LANES=64,            # head.hip dense_fwd_kernel: `k += 64`, dense_bwd_dx_kernel: 64 inputs k per workgroup (the lanes)
    DX_BATCH=16 * 4,     # head.hip dense_bwd_dx_kernel: DXB = 16 loads per wave and round, four waves: `m += 4 * DXB`, then `m += 4`
    DW_KBLOCK=256,       # head.hip dense_bwd_dw_kernel: `k = blockIdx.x * 256 + threadIdx.x`
    DW_NBATCH=8,         # head.hip dense_bwd_dw_kernel: DWB = 8 samples per round, dzs rows rounded up to 8
    SE_ROUND=32,         # se.hip se_fwd_kernel / se_bwd_kernel: `j0 += 32` (four waves of eight rows)
    SE_BATCH=8,          # se.hip: the 8-wide batches of the fc2 / fc1^T loops, `j + 8 <= Wd`, then one row at a time
    SLAB_GROUPS=16,      # se.hip dw_slab_reduce_block: sixteen part groups, `p += 16` in the tail loop
    SLAB_STRIDE=64,      # se.hip dw_slab_reduce_block: four chains of 16 parts, `p += 64`
    ALL_FINITE_CAP=2048,  # head.hip x3d_all_finite: `if (blocks > 2048)`, 256 * 8 elements per workgroup below the cap
    L2_SUMSQ_CAP=1024,   # head.hip x3d_l2_sumsq: `if (blocks > 1024)`
    GRID_Y=65535,        # the 16 bits of gridDim.y (elem.hip elem_grid: N * C planes in y)
)


def aux_tile_defines(csrc=None):
    """{name: value} of AUX_TILE_SOURCES' #define lines, read from the kernel sources; KeyError names a missing one."""
    import os
    import re
    csrc = csrc or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "x3d-tf_amd", "csrc")
    out = {}
    for fname, names in AUX_TILE_SOURCES.items():
        text = open(os.path.join(csrc, fname)).read()
        for nm in names:
            m = re.search(rf"^#define\s+{nm}\s+(\d+)\b", text, re.M)
            if not m:
                raise KeyError(f"{fname}: no `#define {nm} <integer>` line")
            out[nm] = int(m.group(1))
    return out


def aux_vec(dtype):
    return 4 if dtype == F32 else 8


def _aux_edge():
    T, Lt = AUX_TILES, AUX_LITERALS
    E = []
    # dense_fwd (N, K, M, act, mask_scale, bias); dense_bwd (N, K, M, act, mask_scale, dx, db)
    E += [("dense_fwd",) + c for c in [
        (1, 1, 1, 0, None, False), (3, 63, 5, 1, None, True), (8, 64, 4, 0, 2.0, True), (9, 65, 157, 1, 2.0, False),
        (5, 200, 101, 0, None, True), (17, 257, 174, 1, 2.0, True), (37, 630, 51, 0, 2.0, True), (70, 129, 259, 1, None, False),
        (2, 256, 7, 0, None, True)]]
    E += [("dense_bwd",) + c for c in [
        (1, 1, 1, 0, None, True, True), (3, 63, 5, 1, None, True, False),
        (4, 64, 64, 0, 2.0, True, True),        # M = 64: every wave runs its 16-batch exactly once and has no tail
        (5, 65, 61, 1, 2.0, True, True),        # wave 0 takes the batch, waves 1 to 3 only the tail
        (9, 255, 157, 0, 2.0, False, True), (8, 256, 101, 1, None, True, True), (17, 257, 174, 0, None, True, False),
        (70, 300, 259, 1, 2.0, True, True), (130, 54, 400, 0, None, True, True)]]
    # the host limits (64 KiB of LDS): dz [DENSE_BN][M] floats, dzs [N rounded up to 8][DENSE_BM] floats
    E += [("dense_bwd_refused", 1, 1, 65536 // (4 * T["DENSE_BN"]) + 1), ("dense_bwd_refused", 65536 // (4 * T["DENSE_BM"]) + 1, 2, 3)]
    for m in (1, 2, 8, 63, 255, 256, 257, 1000):
        E += [("softmax_xent", n, m, 0.5, True) for n in (1, 3)]
    E += [("softmax_xent", n, m, 1.0, False) for m in (1, 257) for n in (1, 3)]
    E += [("view_mean",) + c for c in [(1, 1, 1), (3, 2, 127), (2, 3, 128), (2, 30, 129), (5, 10, 401)]]
    # squeeze-excite
    E += [("se_fwd",) + c for c in [
        (1, 1, 1, 8), (3, 63, 7, 100), (2, 64, 8, 100), (2, 65, 9, 100), (5, 257, 33, 49), (3, 306, 24, 64), (2, 630, 40, 36),
        (2, T["SE_MAXC"], T["SE_MAXW"], 10), (65, 72, 8, 100)]]
    E += [("se_fwd_refused", 2, T["SE_MAXC"] + 1, 8), ("se_fwd_refused", 2, 24, T["SE_MAXW"] + 1)]
    E += [("se_bnb_bwd",) + c for c in [
        (2, 306, 24, 64, True, ()), (3, 630, 40, 36, True, ()),        # the XL training widths; 40: the second `j0 += 32` round
        (65, 72, 8, 16, True, ()), (130, 24, 0, 16, False, ()), (1, 1, 1, 8, True, ()), (5, 257, 33, 8, True, ((1, 4),)),
        (4, 63, 7, 12, True, ((15, 60), (17, 68))), (3, 40, T["SE_MAXW"], 12, True, ((16, 64), (65, 252))),
        (4, 24, 0, 12, False, ((63, 4), (113, 128))),                  # the 256-thread launch without SE
        (2, T["SE_MAXC"], 16, 8, True, ())]]
    # slab reducer: every (parts, elems), alternately one and two jobs per launch
    combos = [(p, e) for p in (1, 15, 16, 17, 48, 49, 63, 64, 65, 113) for e in (4, 60, 64, 68)]
    i, two = 0, False
    while i < len(combos):
        k = 2 if two and i + 1 < len(combos) else 1
        E.append(("dw_slab_reduce", tuple(combos[i:i + k])))
        i, two = i + k, not two
    E += [("dw_slab_reduce_refused", 3, 6, 0), ("dw_slab_reduce_refused", 3, 8, 1)]
    # plane-wise kernels: every entry at every P edge of its storage type, the second option of each entry in turn
    span = lambda dt: T["ELEM_BLOCK"] * aux_vec(dt) * T["ELEM_ITERS"]      # one workgroup's elements on the vector path
    small = T["ELEM_BLOCK"] * 8                                          # tail_bwd: 16-bit planes below it take the small-plane kernel
    rot = {"tail_bwd": (False, True), "tail_fwd": (None, "identity", "conv"),
           "relu_bn_bwd_reduce": (("dy", True), ("dy", False), ("dpool", True)), "pool_fwd": ((),)}
    cnt = {k: 0 for k in rot}

    def plane(entry, dt, n, c, P, *off):
        o = rot[entry][cnt[entry] % len(rot[entry])]
        cnt[entry] += 1
        E.append((entry, dt, n, c, P) + (o if isinstance(o, tuple) else (o,)) + off)
    for entry in rot:
        for dt in (BF16, F16):
            for P in (8, small - 8, small, small + 8, span(dt) - 8, span(dt), span(dt) + 8):
                plane(entry, dt, 3, 5, P)
        for P in (4, span(F32) - 4, span(F32), span(F32) + 4):
            plane(entry, F32, 3, 5, P)
        s1 = T["ELEM_BLOCK"] * T["ELEM_ITERS"]                             # the scalar path's span
        for dt in (BF16, F16, F32):
            for P in (1, 7, s1 - 1, s1, s1 + 1):
                plane(entry, dt, 3, 5, P)
            plane(entry, dt, 3, 5, s1, 1)                                  # (s1 is a multiple of VEC: scalar only off alignment)
        # views that are not 16-byte aligned although P % VEC == 0: pick_vec's 4 (16-bit) / 2 (fp32) collapse to the scalar kernel
        for dt, P, off in ((BF16, small, 1), (F16, small, 4), (F32, span(F32), 2), (BF16, 8, 1)):
            plane(entry, dt, 2, 3, P, off)
        # N * C planes beyond the 16 bits of gridDim.y (pool_fwd: in gridDim.x)
        plane(entry, BF16, 175, 400, 8)
    E.append(("tail_bwd", F32, 175, 400, 4, True))     # (16-bit planes of 8 take the small-plane kernel, whose grid is (C, N / NB))
    # small-plane groups of tail_bwd, NB = min(1024 // (P / 8), N, 16) samples per workgroup: 16 + 1, 4 + 1, 15 + 1 (the last with
    # two rounds of the 512-vector loop)
    for i, (n, P) in enumerate(((17, 8), (5, small - 8), (16, 520))):
        E += [("tail_bwd", BF16, n, 3, P, i % 2 == 0), ("tail_bwd", F16, n, 3, P, i % 2 == 1)]
    # layout converter: C = 3 and P % 8 == 0 on aligned tensors is the vector form
    pairs = ((F32, F32), (F32, BF16), (BF16, BF16), (BF16, F32), (F32, F16), (F16, F16), (F16, F32))
    E += [("nthwc_to_ncthw", s, d, 2, 3, P) for P in (8, small - 8, small, small + 8) for s, d in pairs]
    E += [("nthwc_to_ncthw", s, d, 2, 3, small - 1) for s, d in pairs[:3]]
    E += [("nthwc_to_ncthw", s, d, 2, 3, small, 1) for s, d in pairs[2:5]]
    E += [("nthwc_to_ncthw",) + pairs[(i + 3) % 7] + (2, c, 300) for i, c in enumerate((1, 2, 4, 24))]
    # grid-stride reductions, below and above their workgroup caps
    kinds = ("+inf", "-inf", "nan", "-nan-payload")
    big = 2048 * Lt["ALL_FINITE_CAP"] + 257
    for n in (1, 63, 2047, 2048, 2049, big):
        E.append(("all_finite", n, "none", "first"))
        pos = ("first",) if n == 1 else ("first", "last", "mid") + (("trip2",) if n == big else ())
        full = n in (2049, big)
        for j, ps in enumerate(pos):
            E += [("all_finite", n, k, ps) for i, k in enumerate(kinds) if full or i == (j + n) % 4]
    E += [("l2_sumsq", n, m) for n in (1, 255, 2049, 2048 * Lt["L2_SUMSQ_CAP"] + 513) for m in (None, "random", "zeros")]
    return E


AUX_EDGE = _aux_edge()
aux_edge_id = aux_full_id          # (defined below AUX_FULL: the same id scheme)


# ---- ROI head (csrc/roi.hip): one case per loop and dispatch class of x3d_roi_pool_fwd / x3d_roi_pool_bwd ------------------------
# (label, (T, H, W), C, K, num_boxes of the two samples, R, sampling_ratio, 1 / spatial_scale, boxes, (x_raw, yraw, g) offsets in
# elements off a 16-byte boundary, extra).  boxes: "grid" = roi_ref.box_mix (1/8-pixel grid), "offgrid" = roi_ref.box_mix_offgrid;
# both cycle through BOX_KINDS over the slots, so every round of four boxes mixes valid, zero-width, NaN and empty ones.
# extra: "poison" = the backward is run a second time with argmax bytes >= R*R in some valid rows.  tests/roi_classes.py restates
# what the launchers and kernels make of a case, and tests/test_roi_head.py fails with the name of a class no case here runs.
_Z = (0, 0, 0)
ROI_EDGE = [
    # the shipped default (MAX_BOXES 8, R 7, sampling_ratio 0) on X3D-M's conv5 plane: 784 elements, 16-bit vectors cross planes of 49
    ("m-default", (16, 7, 7), 24, 8, (8, 5), 7, 0, 32, "grid", _Z, ""),
    # X3D-S: 325 elements, scalar in every type; a sample without boxes next to one with two rounds
    ("s-plane", (13, 5, 5), 3, 8, (8, 0), 7, 0, 32, "grid", _Z, ""),
    # X3D-XS: 100 elements, fp32 vectors and 16-bit scalars; L / XL: planes of 100 pixels, every vector type with H*W % 8 = 4
    ("xs-plane-sr0", (4, 5, 5), 3, 8, (8, 3), 7, 0, 32, "grid", _Z, ""),
    ("xs-plane-sr2", (4, 5, 5), 3, 8, (7, 8), 7, 2, 32, "grid", _Z, ""),
    ("l-plane-sr0", (16, 10, 10), 3, 8, (8, 6), 7, 0, 32, "grid", _Z, ""),
    ("l-plane-sr2", (16, 10, 10), 3, 8, (3, 8), 7, 2, 32, "grid", _Z, ""),
    # box rounds on their own: a second round with one wave at work next to exactly one full round; sixteen rounds, and nine with the
    # count ending inside the last
    ("round2-one-wave", (2, 8, 10), 3, 5, (5, 4), 7, 0, 32, "grid", _Z, "poison"),
    ("rounds-16", (2, 8, 10), 2, 64, (64, 33), 2, 0, 32, "grid", _Z, ""),
    # bins per lane: R*R = 64 fills the wave, 81 gives 17 lanes a second bin, 225 takes four trips
    ("bins-64", (2, 8, 10), 3, 3, (3, 2), 8, 0, 32, "grid", _Z, ""),
    ("bins-81", (2, 8, 10), 3, 3, (2, 3), 9, 2, 32, "grid", _Z, ""),
    ("bins-225", (2, 8, 10), 3, 3, (3, 1), 15, 0, 32, "grid", _Z, ""),
    ("bins-64-1024px", (1, 32, 32), 2, 3, (2, 3), 8, 2, 32, "grid", _Z, ""),
    ("bins-81-1024px", (1, 32, 32), 2, 3, (3, 2), 9, 0, 32, "grid", _Z, ""),
    ("bins-225-1024px", (1, 32, 32), 2, 3, (1, 3), 15, 0, 32, "grid", _Z, ""),
    # staging chunks of the forward with a short last one: q = 1 (8 + 1 slices); H*W = 625 (fp32 q = 4: 12 + 4, 16-bit q = 8: 8 + 8);
    # H*W = 900 (fp32 q = 1: 9 + 1, 16-bit q = 2: 8 + 2); 9207 elements, scalar (8 + 1)
    ("chunks-q1", (9, 32, 32), 2, 2, (2, 1), 2, 2, 32, "grid", _Z, ""),
    ("chunks-hw625", (16, 25, 25), 2, 2, (1, 2), 7, 0, 32, "grid", _Z, ""),
    ("chunks-hw900", (10, 30, 30), 2, 2, (2, 2), 2, 2, 32, "grid", _Z, ""),
    ("chunks-scalar", (9, 31, 33), 2, 2, (2, 1), 7, 0, 32, "grid", _Z, ""),
    # pixels per thread: 289, 513 and 930 pixels give the last thread rows 2, 3 and 4 pixels with a ragged end, over two box rounds
    ("pixels-2", (2, 17, 17), 2, 5, (5, 2), 2, 0, 32, "grid", _Z, ""),
    ("pixels-3", (1, 19, 27), 2, 5, (3, 5), 7, 2, 32, "grid", _Z, ""),
    ("pixels-4", (1, 30, 31), 2, 5, (5, 5), 2, 0, 32, "grid", _Z, ""),
    # an extent that divides but a pointer one element off: the forward's x_raw (and with it the backward's yraw), then g alone
    ("misaligned-x", (8, 4, 4), 3, 3, (3, 2), 2, 2, 32, "grid", (1, 1, 0), ""),
    ("misaligned-g", (8, 4, 4), 3, 3, (2, 3), 7, 0, 32, "grid", (0, 0, 1), ""),
    # geometry off the exact grid: boxes drawn uniformly, spatial_scale 1/16 (exact) and 1/24 (rounded to fp32)
    ("geometry-16", (4, 7, 7), 3, 6, (6, 2), 7, 0, 16, "offgrid", _Z, ""),
    ("geometry-24", (4, 7, 7), 3, 6, (2, 6), 7, 2, 24, "offgrid", _Z, ""),
]


def roi_edge_id(case):
    label, (t, h, w), c, k, nb, r, sr = case[:7]
    return f"{label}-{t}x{h}x{w}-C{c}-K{k}-nb{nb[0]}_{nb[1]}-R{r}-sr{sr}"


# ---- whole-model cases (tests/test_model_gpu.py): variant, N, T, S --------------------------------------------------------
MODEL_TRAIN_FP32 = [
    ("XS", 4, 4, 64), ("S", 2, 13, 64), ("M", 2, 4, 64), ("S", 3, 5, 96),
    ("XS", 2, 4, 78),     # odd extents end to end: 78 -> 39 -> 20 -> 10 -> 5 -> 3 (X3D-L's 39 -> 20 TF-SAME pads, odd stride-2 planes)
    ("M", 2, 16, 112),    # T = 16 and 56 / 28 / 14 / 7 planes: the deep-prefetch depthwise variants (dw_pd.hip) inside the model
    ("S", 1, 2, 160),     # BASELINE config 2's real planes (80 / 40 / 20 / 10 / 5)
    ("S", 8, 13, 160),    # BASELINE config 2 at its real clip size (13 x 160^2), a quarter of its batch: the CPU oracle takes ~10 s
]
MODEL_TRAIN_HALF = [     # teacher-forced block by block, bf16 and fp16 storage
    ("S", 3, 5, 96),      # odd point counts: scalar / generic kernel paths
    ("M", 2, 4, 128),     # every P a multiple of 8, 16-byte aligned rows: the fast paths the benchmark runs
    ("XL", 2, 4, 64),     # XL widths (72/162/306/630...: off the 32-grid, K > 432), 55 blocks, SE parity across stages
    ("L", 1, 2, 312),     # BASELINE config 4's real planes: 156 / 78 / 39 / 20 / 10 (odd 39 -> 20)
    ("S", 1, 13, 91),     # 13 frames on half a 182-pixel test crop: ragged planes (46 / 23 / 12 / 6 / 3) and rows of P % 8 != 0 points at every stage
    ("M", 1, 4, 224),     # BASELINE config 3's own planes (112 / 56 / 28 / 14 / 7) with T % 4 == 0: the exact dw_mx variants, the
                          #   stage-2/3 forward tail fold on real rows, the stem fold at 112^2 -- what bench.py times
]
# config overrides of the detection model on the dilated stride-16 map (test_dilated_res5_gpu, test_trajectory, test_trajectory_gpu)
DILATED_DETECTION = ["NETWORK.RES5_DILATION", 2, "DETECTION.ENABLE", True, "DETECTION.MAX_BOXES", 2,
                     "DETECTION.SPATIAL_SCALE_FACTOR", 16]
MODEL_INFER = [           # variant, views, crops, T, S, dtype
    ("XS", 10, 1, 4, 160, F32), ("S", 2, 1, 13, 96, F32),
    ("XL", 10, 3, 2, 96, F32), ("XL", 10, 3, 2, 96, F16), ("XL", 10, 3, 2, 96, BF16),   # BASELINE config 5: 30 views per video
    ("XL", 2, 1, 8, 96, F16),     # stage 5 with P = 8 x 3 x 3 = 72 points (P % 8 == 0): the sliced 630 -> 280 conv on whole vectors
]


# ----------------------------------------------------------------------------------------------------------------------
# argument structs of the kernel-level cases over address-only operands (the dry-run dispatch only looks at alignment)
# ----------------------------------------------------------------------------------------------------------------------
class _Addr:
    nxt = 0x5000_0000_0000

    @classmethod
    def new(cls):
        cls.nxt += 1 << 32
        return cls.nxt


def _code(dtype):
    from x3d_tf_amd import hip
    return hip.dtype_code(dtype)


def pw_fwd_struct(shape, dtype, panel):
    from x3d_tf_amd import hip
    n, cin, cout, t, h, w, stride, pro = shape
    A = _Addr.new
    if pro in ("tail", "tail_conv", "tail1"):
        return hip.PwFwdArgs(A(), A(), A(), A(), A(), None, 1, n, cin, cout, t, h, w, stride, _code(dtype), A() if panel else None,
                             in_add=None if pro == "tail1" else A(), in_add_scale_shift=A() if pro == "tail_conv" else None, in_store=A())
    return hip.PwFwdArgs(A(), A(), A(), A(), A() if pro else None, A() if pro == "swish" else None,
                         {None: 0, "relu": 1, "swish": 2}[pro], n, cin, cout, t, h, w, stride, _code(dtype),
                         A() if panel else None)


def pw_fwd_infer_struct(shape, dtype, panel):
    from x3d_tf_amd import hip
    n, cin, cout, t, h, w, pro, res, oact = shape
    A = _Addr.new
    return hip.PwFwdArgs(A(), A(), A(), None, A() if pro else None, A() if pro == "swish" else None,
                         {None: 0, "relu": 1, "swish": 2}[pro], n, cin, cout, t, h, w, 1, _code(dtype),
                         A() if panel else None, out_scale_shift=A(), out_add=A() if res else None,
                         out_add_scale_shift=A() if res == "conv" else None, out_act=1 if oact == "relu" else 0)


def pw_dgrad_struct(shape, epi, dtype, panel):
    from x3d_tf_amd import hip
    n, cin, cout, t, h, w = shape
    A = _Addr.new
    e = PW_DGRAD_EPI.index(epi)
    sw = epi == "swish_bwd"
    return hip.PwDgradArgs(A(), A(), A(), A(), A(), e, A() if epi in ("add", "add_strided") else None,
                           A() if sw else None, A() if sw else None, A() if sw else None, A() if sw else None,
                           n, cin, cout, t, h, w, _code(dtype), A() if panel else None)


def pw_wgrad_struct(shape, dtype):
    from x3d_tf_amd import hip
    n, cin, cout, t, h, w, stride, pro = shape
    A = _Addr.new
    return hip.PwWgradArgs(A(), A(), A(), A(), A() if pro else None, A() if pro else None, 2 if pro else 0, A(),
                           n, cin, cout, t, h, w, stride, _code(dtype))


def pw_bwd_struct(shape, dtype):
    from x3d_tf_amd import hip
    n, cin, cout, t, h, w, epi = shape[:7]
    tail = shape[7] if len(shape) > 7 else 0
    A = _Addr.new
    e = PW_DGRAD_EPI.index(epi)
    sw = epi == "swish_bwd"
    return hip.PwBwdArgs(A(), A(), A(), A(), A(), e, None if sw else A(), A() if sw else None, A() if sw else None,
                         A() if sw else None, A() if sw else None, None if sw else A(), A(), n, cin, cout, t, h, w,
                         _code(dtype), A() if tail else None, A() if tail == 2 else None, A() if tail else None,
                         A() if tail == 2 else None)


def pw_bwd_rc_struct(shape, dtype):
    from x3d_tf_amd import hip
    n, cin, cout, t, h, w, epi, tail = shape
    A = _Addr.new
    return hip.PwBwdArgs(A(), None, None, None, A(), PW_DGRAD_EPI.index(epi), None if epi == "store" else A(), None, None, None, None, A(), None, n, cin,
                         cout, t, h, w, _code(dtype), A() if tail else None, A() if tail == 2 else None, A() if tail else None,
                         A() if tail == 2 else None, A(), A(), A())


def pw_bwd_rc_strided_struct(shape, dtype):
    from x3d_tf_amd import hip
    n, cin, cout, t, xh, xw = shape
    A = _Addr.new
    return hip.PwBwdArgs(A(), None, None, None, A(), 0, None, None, None, None, None, A(), None, n, cin, cout, t, (xh + 1) // 2,
                         (xw + 1) // 2, _code(dtype), None, None, None, None, A(), A(), A(), 2, xh, xw)


def dw_fwd_struct(shape, dtype):
    from x3d_tf_amd import hip
    n, c, t, h, w, stride = shape
    A = _Addr.new
    return hip.Dw3dFwdArgs(A(), A(), A(), A(), 1, A(), A(), n, c, t, h, w, stride, _code(dtype))


def dw_full_struct(case):
    """The argument struct of a DW_FULL case over address-only operands, in the case's launch form."""
    from x3d_tf_amd import hip
    e, dtype, n, c, t, h, w, stride, pro, st, pool = case
    A = _Addr.new
    if e == "bwd":
        return dw_bwd_struct((n, c, t, h, w, stride), dtype)
    fold = hip.BnFold(A(), 1.0, A(), A(), A(), A(), 1e-5, 0.9, 1, A(), A()) if pro == "bn" else None
    a = hip.Dw3dFwdArgs(A(), A(), A(), None if fold else A(), 1, A() if st else None, A() if pool else None, n, c, t, h, w,
                        stride, _code(dtype), None if fold is None else __import__("ctypes").pointer(fold))
    a._fold = fold           # (the struct holds a raw pointer to it)
    return a


def dw_bwd_struct(shape, dtype):
    from x3d_tf_amd import hip
    n, c, t, h, w, stride = shape
    A = _Addr.new
    return hip.Dw3dBwdArgs(A(), A(), A(), A(), A(), A(), A(), A(), A(), n, c, t, h, w, stride, _code(dtype))
