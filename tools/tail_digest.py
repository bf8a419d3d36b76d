"""SHA-256 of the output buffers of the five residual-tail entry points (csrc/elem.hip: x3d_tail_fwd, x3d_tail_fwd_bn, x3d_tail_fwd_dp,
x3d_tail_bwd, x3d_tail_bwd_dp) on fixed inputs: the bit-identity record of a refactor.

    python tools/tail_digest.py                                   print the digests of the current build
    python tools/tail_digest.py --record FILE --commit HASH --hipcc "LINE"
                                                                  write them as tests/golden/tail_bits.json holds them

`digests(gpu)` is the one place that builds the inputs, makes the calls and hashes the raw bytes of y, g (in place), g_branch,
sums_c, sums_r and, for x3d_tail_fwd_bn, the coefficient and moving-statistics tables; tests/test_tail_bits_gpu.py calls it and
compares with the recorded file.  X3D_HIP_LIB selects the library (hip.py), so a record is taken with the library of the commit it
names.  Every output buffer is filled with a sentinel (123; the fp64 accumulators 0.25) before the call and hashed whole after it,
the padding of a misaligned buffer included, so a store that goes missing or strays shows as much as one that changes.

Storage  fp32, fp16, bf16; VEC = the full vector (4 fp32 / 8 16-bit elements) or scalars.
Shapes   general kernels, (N, C, P): (1, 1, VEC) one vector; (3, 3, 256 * 4 * VEC + VEC) a second workgroup per plane holding one
         vector; the same with the scalar chunk, (3, 3, 1024 + VEC) behind pointers one element off a 16-byte boundary ("io": y and
         the shortcut forward, dy_g backward); (3, 3, 1027) odd P, scalars; 16-bit (2, 2, 2048), P / 8 = 256, the first plane the
         general backward takes.  Small-plane backward, 16-bit: (1, 1, 8); (3, 2, 24); (17, 2, 392), the 7 x 7 x 8 plane, NB = 16:
         two groups, the second of one sample, two rounds of the two-vector loop.
Forms    forward: r_scale_shift (r_bn) null and given, x3d_tail_fwd also without a shortcut; backward: r_raw null and given;
         x3d_tail_bwd_dp also with g_branch as the only misaligned pointer ("gbr", which makes the launch scalar), on the two-workgroup
         shape and on (3, 2, 24); x3d_tail_bwd on (3, 2, 24) under X3D_TAIL_SMALL=0 (read by builds with -DX3D_EXPERIMENTS only: the
         product library runs the small-plane kernel again; the case is dyadic, so both paths give the same bits).
Keep     the drop-path forms under four tables: all kept, alternating, all dropped, only the last sample kept.  The c_raw of every
         dropped sample is NaN: it must not be loaded.
Inputs   two families, because fp64 atomics from several workgroups arrive in no fixed order.
         random   normal values, keep in {0, 1.25}.  The elementwise outputs are hashed always, the sums only where exactly one
                  workgroup adds to each channel (N = 1 with one chunk; the small-plane kernel with N <= NB): that pins the order of
                  the reduction inside a workgroup and the contraction into FMAs.
         dyadic   activations and gradients multiples of 1/8 up to 4 in magnitude, scales and shifts multiples of 1/4, keep in
                  {0, 2}: every product and partial sum is exact in fp32 and every total in fp64 whatever the order, so the sums
                  are hashed in every case.  _dyadic_bound() asserts on the host that the largest |term| times the terms of one
                  workgroup stays below 2^24 units of the terms' grid."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
FULL = {"f32": 4, "f16": 8, "bf16": 8}
BLOCK, ITERS = 256, 4                      # ELEM_BLOCK, ELEM_ITERS of elem.hip
SMALL = ((1, 1, 8), (3, 2, 24), (17, 2, 392))
FAMILIES = ("random", "dyadic")
KEEPS = ("all", "alternating", "none", "last")
SENTINEL = 123.0


def general_cases(dt):
    v = FULL[dt]
    cases = [(1, 1, v, None), (3, 3, BLOCK * ITERS * v + v, None), (3, 3, BLOCK * ITERS + v, "io"), (3, 3, 1027, None)]
    return cases + ([(2, 2, 2048, None)] if dt != "f32" else [])


def _launch_of_bwd(dt, n, p, misaligned, small_ok=True):
    """(elements one workgroup of the backward sums in fp32, workgroups that add to one channel): the rule of elem.hip"""
    vec = FULL[dt] if p % FULL[dt] == 0 and not misaligned else 1
    if small_ok and dt != "f32" and vec == 8 and p // 8 < BLOCK:
        nb = min(4 * BLOCK // (p // 8), n, 16)
        return nb * p, -(-n // nb)
    chunk = BLOCK * ITERS * vec
    return min(p, chunk), n * -(-p // chunk)


def _dyadic_bound(dt, n, p, misaligned):
    """The terms of a workgroup's sums in units of their own grids: g on 1/8 up to 4, 32 units, and so gb = keep * g on keep / 8
    (keep a power of two: gb is exact in the storage type as well); gb * c_raw and g * r_raw on the product of two such grids up to
    the product of the bounds, 32 * 32 units.  Largest |term| x terms of one workgroup < 2^24: every partial sum is exact in fp32."""
    for small_ok in (True, False):
        terms, _ = _launch_of_bwd(dt, n, p, misaligned, small_ok)
        assert 32 * 32 * terms < 2 ** 24, f"dyadic case {(dt, n, p)}: 1024 units x {terms} terms is not below 2^24"


def _inputs(dt, n, c, p, family):
    """host tensors of one shape in the storage type: c_raw, shortcut / r_raw, dy, y of the backward; fp32 [C][2] coefficients"""
    rng = np.random.RandomState((1000003 * n + 1009 * c + p + (7 if family == "dyadic" else 1)) % (2 ** 31))
    if family == "random":
        act = lambda: torch.from_numpy(rng.randn(n, c, p).astype(np.float32)).to(DTYPES[dt])
        coef = lambda: torch.from_numpy(np.stack([rng.rand(c) + 0.5, rng.randn(c)], 1).astype(np.float32)).contiguous()
    else:
        act = lambda: torch.from_numpy((rng.randint(-32, 33, size=(n, c, p)) / 8.0).astype(np.float32)).to(DTYPES[dt])
        coef = lambda: torch.from_numpy((rng.randint(-8, 9, size=(c, 2)) / 4.0).astype(np.float32)).contiguous()
    d = dict(c_raw=act(), sh=act(), dy=act(), y=torch.relu(act()), ss_c=coef(), ss_r=coef())
    # the folded BatchNorm of x3d_tail_fwd_bn: exact totals of a made-up mean and variance (no host reduction to reproduce)
    for b in ("c", "r"):
        mean, var = rng.randint(-8, 9, size=c) / 8.0, rng.randint(1, 17, size=c) / 8.0
        d["bn_" + b] = dict(stats=torch.from_numpy(np.stack([n * p * mean, n * p * (var + mean * mean)], 1).astype(np.float64)).contiguous(),
                            gamma=torch.from_numpy((1.0 + rng.randint(-4, 5, size=c) / 8.0).astype(np.float32)),
                            beta=torch.from_numpy((rng.randint(-8, 9, size=c) / 8.0).astype(np.float32)))
    return d


def _keep(n, pattern, value):
    k = torch.zeros(n)
    if pattern == "all":
        k[:] = value
    elif pattern == "alternating":
        k[0::2] = value
    elif pattern == "last":
        k[-1] = value
    return k


def _place(t, gpu, off):
    """(view, whole buffer) of t on the GPU; off: the view starts one element past a 16-byte boundary, inside a sentinel-filled buffer"""
    if not off:
        v = t.to(gpu)
        return v, v
    base = torch.full((t.numel() + 8,), SENTINEL, dtype=t.dtype, device=gpu)
    v = base[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v, base


def _sentinel(shape, dtype, gpu, off=False):
    return _place(torch.full(shape, SENTINEL, dtype=dtype), gpu, off)


def _sha(bufs):
    h = hashlib.sha256()
    for name, buf in bufs:
        h.update(name.encode() + b"\0")
        h.update(memoryview(buf.cpu().contiguous().view(torch.uint8).numpy().reshape(-1)))
    return h.hexdigest()


def _poisoned(c_raw, keep):
    out = c_raw.clone()
    out[keep == 0] = float("nan")
    return out


def _forward(ops, gpu, out, dt, case, family, H):
    n, c, p, off = case
    dtype, tag = DTYPES[dt], f"{dt}/N{case[0]}C{case[1]}P{case[2]}/{off or 'aligned'}/{family}"
    kv = 1.25 if family == "random" else 2.0
    c_raw, ss_c, ss_r = H["c_raw"].to(gpu), H["ss_c"].to(gpu), H["ss_r"].to(gpu)
    sh, _ = _place(H["sh"], gpu, off)
    for form in ("stem", "identity", "conv"):
        y, y_all = _sentinel((n, c, p), dtype, gpu, off)
        ops.tail_fwd(c_raw, ss_c, None if form == "stem" else sh, ss_r if form == "conv" else None, y)
        out[f"tail_fwd/{tag}/{form}"] = _sha([("y", y_all)])
    for form in ("identity", "conv"):
        y, y_all = _sentinel((n, c, p), dtype, gpu, off)
        tables, folds, live = [], [], []                  # (live: the fold structs hold raw pointers)
        for b in ("c", "r") if form == "conv" else ("c",):
            bn = {k: v.to(gpu) for k, v in H["bn_" + b].items()}
            t = dict(mm=torch.full((c,), -0.5, device=gpu), mv=torch.full((c,), 2.0, device=gpu),
                     ss=torch.full((c, 2), SENTINEL, device=gpu), mi=torch.full((c, 2), SENTINEL, device=gpu))
            folds.append(ops.bn_fold(bn["stats"], n * p, bn["gamma"], bn["beta"], t["mm"], t["mv"], 1e-5, 0.9, 1, t["ss"], t["mi"]))
            live.append(bn)
            tables += [(f"{b}_{k}", v) for k, v in t.items()]
        ops.tail_fwd_bn(c_raw, folds[0], sh, folds[1] if form == "conv" else None, y)
        out[f"tail_fwd_bn/{tag}/{form}"] = _sha([("y", y_all)] + tables)
    for form in ("identity", "conv"):
        for pattern in KEEPS:
            keep = _keep(n, pattern, kv)
            y, y_all = _sentinel((n, c, p), dtype, gpu, off)
            ops.tail_fwd_dp(_poisoned(H["c_raw"], keep).to(gpu), ss_c, sh, ss_r if form == "conv" else None, keep.to(gpu), y)
            out[f"tail_fwd_dp/{tag}/{form}/keep_{pattern}"] = _sha([("y", y_all)])


def _backward(ops, gpu, out, dt, case, family, H, dp_only=False, small_ok=True):
    """off: None, "io" (dy_g misaligned) or "gbr" (x3d_tail_bwd_dp only: g_branch misaligned)"""
    n, c, p, off = case
    dtype, tag = DTYPES[dt], f"{dt}/N{case[0]}C{case[1]}P{case[2]}/{off or 'aligned'}/{family}"
    kv = 1.25 if family == "random" else 2.0
    if family == "dyadic":
        _dyadic_bound(dt, n, p, off is not None)
    _, wgs = _launch_of_bwd(dt, n, p, off is not None, small_ok)
    with_sums = family == "dyadic" or wgs == 1
    y, r_raw = H["y"].to(gpu), H["sh"].to(gpu)

    def sums():
        return torch.full((c, 2), 0.25, dtype=torch.float64, device=gpu)
    for form in ("identity", "conv"):
        rr = r_raw if form == "conv" else None
        if not dp_only:
            g, g_all = _place(H["dy"], gpu, off == "io")
            sc, sr = sums(), (sums() if rr is not None else None)
            ops.tail_bwd(g, y, H["c_raw"].to(gpu), rr, sc, sr)
            bufs = [("g", g_all)] + ([("sums_c", sc)] + ([("sums_r", sr)] if sr is not None else []) if with_sums else [])
            out[f"tail_bwd/{tag}/{form}" + ("" if small_ok else "/X3D_TAIL_SMALL=0")] = _sha(bufs)
        if not small_ok:
            continue
        for pattern in KEEPS:
            keep = _keep(n, pattern, kv)
            g, g_all = _place(H["dy"], gpu, off == "io")
            gb, gb_all = _sentinel((n, c, p), dtype, gpu, off == "gbr")
            sc, sr = sums(), (sums() if rr is not None else None)
            ops.tail_bwd_dp(g, gb, y, _poisoned(H["c_raw"], keep).to(gpu), rr, keep.to(gpu), sc, sr)
            bufs = [("g", g_all), ("g_branch", gb_all)] + ([("sums_c", sc)] + ([("sums_r", sr)] if sr is not None else []) if with_sums else [])
            out[f"tail_bwd_dp/{tag}/{form}/keep_{pattern}"] = _sha(bufs)


def digests(gpu):
    """{entry: sha256 hex} in a fixed order (insertion order of the dict)"""
    from x3d_tf_amd import ops
    out = {}
    for dt in DTYPES:
        for family in FAMILIES:
            for case in general_cases(dt):
                H = _inputs(dt, case[0], case[1], case[2], family)
                _forward(ops, gpu, out, dt, case, family, H)
                _backward(ops, gpu, out, dt, case, family, H)
            two_wg = general_cases(dt)[1]
            gbr_cases = [two_wg[:3] + ("gbr",)]
            if dt != "f32":
                for n, c, p in SMALL:
                    _backward(ops, gpu, out, dt, (n, c, p, None), family, _inputs(dt, n, c, p, family))
                gbr_cases.append(SMALL[1] + ("gbr",))
            for case in gbr_cases:
                _backward(ops, gpu, out, dt, case, family, _inputs(dt, case[0], case[1], case[2], family), dp_only=True)
        if dt != "f32":
            n, c, p = SMALL[1]
            before = os.environ.get("X3D_TAIL_SMALL")
            os.environ["X3D_TAIL_SMALL"] = "0"
            try:
                _backward(ops, gpu, out, dt, (n, c, p, None), "dyadic", _inputs(dt, n, c, p, "dyadic"), small_ok=False)
            finally:
                if before is None:
                    del os.environ["X3D_TAIL_SMALL"]
                else:
                    os.environ["X3D_TAIL_SMALL"] = before
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", metavar="FILE", help="write the fixture here instead of printing the digests")
    ap.add_argument("--commit", help="the commit the library in use was built from (--record)")
    ap.add_argument("--hipcc", help="the `hipcc --version` line of the compiler it was built with (--record)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tail_digest.py runs the kernels: it needs the GPU"
    d = digests(torch.device("cuda:0"))
    if not args.record:
        for k, v in d.items():
            print(v, k)
        return
    assert args.commit and args.hipcc, "--record needs --commit and --hipcc: the digests belong to that source and compiler"
    with open(args.record, "w") as fh:
        json.dump(dict(commit=args.commit, hipcc=args.hipcc, device=torch.cuda.get_device_name(0), digests=d), fh, indent=1)
        fh.write("\n")
    print(f"{len(d)} digests -> {args.record}")


if __name__ == "__main__":
    main()
