"""The dispatch rules of the dense convolutions as a table: one shape on each side of every threshold, the rule quoted
beside the rows.  tests/test_conv_plan_cpu.py asks the host-only queries (sr_conv2d_path, sr_conv2d_wgrad_path) for every
row; tests/test_dispatch_edges_gpu.py launches the rows marked on_gpu and compares the kernels that ran."""
import make_golden_conv_plan as G
from stylerenderer_amd import _lib as P

SWITCHES = sorted({name for name, _ in G.SETTINGS})      # every switch a row may set
MISALIGNED = 4            # a pointer that is not 16-byte aligned; the queries never dereference it
STRIPS = P.CONV_PATH_STRIPS

# (geometry, (B, C, N, IH, IW), switches, input pointer, have_scratch, path, on_gpu)
# on_gpu: the shape is one of the GPU suite's (test_conv_gpu, test_conv_s2_wino_gpu, test_dispatch_edges_gpu) or the
# 32^2 512 -> 512 layer; test_dispatch_edges_gpu launches those and compares the kernels that ran with `path`.
FORWARD = [
    # 3x3 stride 1 pad 1 — Winograd iff H % 8 == 0 && W % 32 == 0 && C % 8 == 0 && C <= 512 && N % 64 == 0, 16-byte
    # aligned input / output, a scratch, SR_WINOGRAD != 0
    ("c3", (1, 8, 64, 8, 32), {}, None, 1, P.CONV_PATH_WINO, True),
    ("c3", (1, 64, 64, 32, 48), {}, None, 1, P.CONV_PATH_DIRECT, False),          # W % 32 = 16
    ("c3", (1, 64, 64, 12, 32), {}, None, 1, P.CONV_PATH_DIRECT, False),          # H % 8 = 4
    ("c3", (2, 12, 140, 64, 64), {}, None, 1, P.CONV_PATH_DIRECT, True),          # C % 8 = 4 (and N % 64 = 12)
    ("c3", (1, 64, 96, 32, 32), {}, None, 1, P.CONV_PATH_DIRECT, False),          # N % 64 = 32
    ("c3", (2, 512, 64, 8, 32), {}, None, 1, P.CONV_PATH_WINO, True),             # C = 512: the largest style row
    ("c3", (2, 520, 64, 8, 32), {}, None, 1, P.CONV_PATH_DIRECT, False),          # C > 512
    ("c3", (1, 8, 64, 8, 32), {}, MISALIGNED, 1, P.CONV_PATH_DIRECT, False),      # misaligned input
    ("c3", (1, 8, 64, 8, 32), {}, None, 0, P.CONV_PATH_DIRECT, False),            # no scratch for the transformed weights
    ("c3", (1, 8, 64, 8, 32), {"SR_WINOGRAD": "0"}, None, 1, P.CONV_PATH_DIRECT, True),
    # 3x3 stride 2 pad 0 — polyphase Winograd iff IH = 2 OH + 1, OW % 32 == 0, OH % 8 == 0, C % 4 == 0, N % 64 == 0,
    # aligned buffers, a scratch, and workgroups B * (OW / 32) * (OH / 8) * (N / 64) >= 192 (or SR_CONV_S2_WINO=force)
    ("c3s2", (6, 64, 512, 65, 65), {}, None, 1, P.CONV_PATH_S2_WINO, False),      # 6 * 1 * 4 * 8 = 192
    ("c3s2", (5, 64, 512, 65, 65), {}, None, 1, P.CONV_PATH_DIRECT, False),       # 160
    ("c3s2", (5, 64, 512, 65, 65), {"SR_CONV_S2_WINO": "force"}, None, 1, P.CONV_PATH_S2_WINO, False),
    ("c3s2", (2, 64, 64, 129, 129), {}, None, 1, P.CONV_PATH_DIRECT, True),       # 2 * 2 * 8 * 1 = 32
    ("c3s2", (2, 64, 64, 129, 129), {"SR_CONV_S2_WINO": "force"}, None, 1, P.CONV_PATH_S2_WINO, True),
    ("c3s2", (6, 64, 512, 65, 65), {"SR_CONV_S2_WINO": "0"}, None, 1, P.CONV_PATH_DIRECT, False),
    ("c3s2", (6, 64, 512, 65, 65), {}, MISALIGNED, 1, P.CONV_PATH_DIRECT, False),
    ("c3s2", (6, 64, 512, 65, 65), {}, None, 0, P.CONV_PATH_DIRECT, False),
    ("c3s2", (6, 64, 512, 64, 64), {}, None, 1, P.CONV_PATH_DIRECT, False),       # IH != 2 OH + 1 (OH = 31)
    ("c3s2", (6, 64, 512, 65, 65), {"SR_CONV_SPLIT_BF16": "1"}, None, 1, P.CONV_PATH_S2_BF16, False),   # opt-in, first
    # 1x1 stride 1 pad 0 — GEMM iff C % 16 == 0, N % 128 == 0, pixels % 128 == 0, aligned operands and tiles
    # (P / 128) * (N / 128) * B >= 256; it needs no scratch
    ("c1", (4, 64, 256, 64, 64), {}, None, 1, P.CONV_PATH_GEMM1X1, True),         # 32 * 2 * 4 = 256
    ("c1", (4, 64, 256, 64, 62), {}, None, 1, P.CONV_PATH_DIRECT, True),          # 31 * 2 * 4 = 248
    ("c1", (7, 512, 512, 32, 32), {}, None, 1, P.CONV_PATH_DIRECT, False),        # 8 * 4 * 7 = 224
    ("c1", (8, 512, 512, 32, 32), {}, None, 0, P.CONV_PATH_GEMM1X1, False),       # 256, without a scratch
    ("c1", (8, 512, 64, 32, 32), {}, None, 1, P.CONV_PATH_DIRECT, False),         # N % 128 = 64
    ("c1", (8, 512, 512, 32, 32), {}, MISALIGNED, 1, P.CONV_PATH_DIRECT, False),
    ("c1", (8, 512, 512, 32, 32), {"SR_CONV1X1_GEMM": "0"}, None, 1, P.CONV_PATH_DIRECT, False),
    ("c1s2", (8, 512, 512, 32, 32), {}, None, 1, P.CONV_PATH_DIRECT, False),      # 1x1 stride 2: always direct
    # transposed 3x3 stride 2 — tap-split iff 18 * B * C * N * IH * IW < 1.05e10 (SR_CONVT_TAPS=1: always, =0: never)
    ("t3s2", (2, 512, 512, 32, 32), {}, None, 1, P.CONV_PATH_CONVT_TAPS, False),  # 9.66e9
    ("t3s2", (4, 512, 512, 32, 32), {}, None, 1, P.CONV_PATH_CONVT_FUSED_KS | STRIPS, False),   # 1.93e10
    ("t3s2", (4, 512, 512, 8, 8), {}, None, 1, P.CONV_PATH_CONVT_TAPS, True),
    ("t3s2", (2, 512, 512, 32, 32), {}, None, 0, P.CONV_PATH_DIRECT, False),      # no scratch: no taps, no K slices
    ("t3s2", (8, 512, 512, 32, 32), {"SR_CONVT_TAPS": "1"}, None, 1, P.CONV_PATH_CONVT_TAPS, False),
    # ... else the interior by k_convt_fused iff IW >= 16, IH % 4 == 0, IW % 32 == 0, C % 8 == 0, aligned input and
    # (fused_blocks = (IW / 32) * (IH / 4) * ceil(N / 128) * B >= 192 || C <= 256); with fewer blocks and more channels
    # in the smallest of 2 / 4 K slices with C % (16 ks) == 0, C / ks >= 64, fused_blocks * ks >= 192
    ("t3s2", (8, 512, 512, 32, 32), {}, None, 1, P.CONV_PATH_CONVT_FUSED | STRIPS, True),                    # 256 blocks
    ("t3s2", (2, 256, 512, 32, 32), {"SR_CONVT_TAPS": "0"}, None, 1, P.CONV_PATH_CONVT_FUSED | STRIPS, False),   # 64, C <= 256
    ("t3s2", (2, 320, 512, 32, 32), {"SR_CONVT_TAPS": "0"}, None, 1, P.CONV_PATH_CONVT_FUSED_KS | STRIPS, True),  # 64 * 4
    ("t3s2", (4, 512, 256, 32, 32), {"SR_CONVT_TAPS": "0"}, None, 1, P.CONV_PATH_CONVT_FUSED_KS | STRIPS, True),  # 64 * 4
    ("t3s2", (1, 512, 512, 32, 32), {"SR_CONVT_TAPS": "0"}, None, 1, P.CONV_PATH_DIRECT, False),             # 32 * 4 < 192
    ("t3s2", (2, 320, 512, 32, 32), {"SR_CONVT_TAPS": "0", "SR_CONVT_FUSED_KS": "0"}, None, 1, P.CONV_PATH_DIRECT, True),
    ("t3s2", (2, 320, 512, 32, 32), {"SR_CONVT_TAPS": "0", "SR_CONVT_FUSED_KS": "0", "SR_CONVT_FUSED": "1"}, None, 1,
     P.CONV_PATH_CONVT_FUSED | STRIPS, False),                                                               # forced, one slice
    ("t3s2", (8, 512, 512, 32, 32), {"SR_CONVT_FUSED": "0"}, None, 1, P.CONV_PATH_DIRECT, False),
    ("t3s2", (8, 512, 512, 32, 32), {}, MISALIGNED, 1, P.CONV_PATH_DIRECT, False),
    ("t3s2", (8, 512, 512, 32, 32), {"SR_CONV_SPLIT_BF16": "1"}, None, 1, P.CONV_PATH_CONVT_BF16 | STRIPS, False),
    ("t3s2", (2, 512, 512, 32, 32), {"SR_CONV_SPLIT_BF16": "1"}, None, 1, P.CONV_PATH_CONVT_BF16 | STRIPS, False),  # no taps
    # IW < 16: no interior kernel, one whole-grid launch per phase
    ("t3s2", (2, 8, 6, 8, 8), {"SR_CONVT_TAPS": "0"}, None, 1, P.CONV_PATH_DIRECT, True),
    ("t3s2", (4, 512, 512, 8, 8), {"SR_CONVT_TAPS": "0", "SR_CONVT_FUSED": "1"}, None, 1, P.CONV_PATH_DIRECT, False),
    # the border behind an interior kernel: strips iff a scratch and SR_CONVT_STRIPS != 0, else per-phase launches
    ("t3s2", (8, 512, 512, 32, 32), {"SR_CONVT_STRIPS": "0"}, None, 1, P.CONV_PATH_CONVT_FUSED, True),
    ("t3s2", (8, 512, 512, 32, 32), {}, None, 0, P.CONV_PATH_CONVT_FUSED, False),
]

# (geometry, (B, C, N, IH, IW), switches, x pointer, path, on_gpu)
WGRAD = [
    # 3x3 stride 1 pad 1 with C <= 4 && N <= 4: streaming kernel (SR_WGRAD_SMALL=0: off)
    ("c3", (4, 3, 3, 64, 64), {}, None, P.WGRAD_PATH_SMALL3, True),
    ("c3", (4, 5, 3, 64, 64), {}, None, P.WGRAD_PATH_DIRECT, False),
    ("c3", (4, 3, 5, 64, 64), {}, None, P.WGRAD_PATH_DIRECT, False),
    ("c3", (4, 3, 3, 64, 64), {"SR_WGRAD_SMALL": "0"}, None, P.WGRAD_PATH_DIRECT, True),
    # ... Winograd iff H % 2 == 0, W % 16 == 0, C % 64 == 0, N % 64 == 0, B <= 32, aligned x / gy, SR_WINOGRAD != 0
    ("c3", (2, 128, 64, 16, 16), {}, None, P.WGRAD_PATH_WINO, True),
    ("c3", (32, 64, 64, 4, 16), {}, None, P.WGRAD_PATH_WINO, True),
    ("c3", (33, 64, 64, 4, 16), {}, None, P.WGRAD_PATH_DIRECT, False),            # B > 32
    ("c3", (2, 128, 64, 16, 24), {}, None, P.WGRAD_PATH_DIRECT, False),           # W % 16 = 8
    ("c3", (2, 128, 64, 15, 16), {}, None, P.WGRAD_PATH_DIRECT, False),           # H odd
    ("c3", (2, 96, 64, 16, 16), {}, None, P.WGRAD_PATH_DIRECT, False),            # C % 64 = 32
    ("c3", (2, 128, 96, 16, 16), {}, None, P.WGRAD_PATH_DIRECT, False),           # N % 64 = 32
    ("c3", (2, 128, 64, 16, 16), {}, MISALIGNED, P.WGRAD_PATH_DIRECT, False),
    ("c3", (2, 128, 64, 16, 16), {"SR_WINOGRAD": "0"}, None, P.WGRAD_PATH_DIRECT, True),
    # 3x3 stride 2 pad 0, either direction (G = the smaller map, U channels = C | N transposed, V channels the other):
    # k_wgrad_s2_dma iff GW % 16 == 0, GH % 4 == 0, U channels % 32 == 0, V channels % 128 == 0, SR_WGRAD_DMA != 0
    ("t3s2", (2, 128, 32, 16, 16), {}, None, P.WGRAD_PATH_S2_DMA, True),
    ("c3s2", (2, 32, 128, 33, 33), {}, None, P.WGRAD_PATH_S2_DMA, True),
    ("t3s2", (2, 128, 32, 16, 16), {"SR_WGRAD_DMA": "0"}, None, P.WGRAD_PATH_DIRECT, True),
    ("c3s2", (2, 32, 64, 33, 33), {}, None, P.WGRAD_PATH_DIRECT, False),          # V channels % 128 = 64
    ("t3s2", (2, 128, 48, 16, 16), {}, None, P.WGRAD_PATH_DIRECT, False),         # U channels % 32 = 16
    ("t3s2", (2, 8, 6, 8, 8), {}, None, P.WGRAD_PATH_DIRECT, True),               # GW % 16 = 8
    # 1x1: direct; the split-bf16 forms are opt-in
    ("c1", (2, 16, 5, 32, 32), {}, None, P.WGRAD_PATH_DIRECT, True),
    ("c1s2", (2, 6, 4, 9, 9), {}, None, P.WGRAD_PATH_DIRECT, True),
    ("c1", (2, 16, 5, 32, 32), {"SR_CONV_SPLIT_BF16": "1"}, None, P.WGRAD_PATH_BF16_1X1, False),
    ("c1", (2, 16, 5, 32, 32), {"SR_CONV_SPLIT_BF16": "1"}, MISALIGNED, P.WGRAD_PATH_DIRECT, False),
    # (its stride-2 form: GW % 32 == 0, U channels % 64 == 0, V channels % 128 == 0)
    ("t3s2", (2, 128, 64, 32, 32), {"SR_CONV_SPLIT_BF16": "1"}, None, P.WGRAD_PATH_BF16_S2, False),
    ("t3s2", (2, 128, 32, 16, 16), {"SR_CONV_SPLIT_BF16": "1"}, None, P.WGRAD_PATH_S2_DMA, False),   # GW % 32 = 16
    ("t3s2", (2, 128, 64, 32, 32), {"SR_CONV_SPLIT_BF16": "c"}, None, P.WGRAD_PATH_S2_DMA, False),   # another family's letter
]


def conv_args(geom, shape):
    """(B, C, N, IH, IW, OH, OW, ksize, stride, pad, transposed) of a table row."""
    k, stride, pad, tr = G.GEOM[geom]
    b, c, n, ih, iw = shape
    return (b, c, n, ih, iw) + G.out_size(ih, iw, k, stride, pad, tr) + (k, stride, pad, tr)


def case_id(row):
    return "%s-B%d-C%d-N%d-%dx%d-%s" % ((row[0],) + row[1] + ("-".join("%s=%s" % kv for kv in row[2].items()) or "unset",))
