"""Every kernel instantiation the BASELINE configurations launch at full size has an oracle-parity case under `-m gpu`.

Runs on the CPU: the library's dispatch is asked in dry-run mode (x3d_pw_kernel_name / x3d_dw3d_kernel_name, nothing is
launched) which instantiation each launch of a full-size DRY plan runs (x3d_tf_amd/dispatch.py), and which instantiation
each registered parity case (tests/shapes.py: the lists tests/test_kernels_gpu.py and tests/test_model_gpu.py
parametrise over) runs.  The first set must be contained in the second.
"""
import functools

import pytest
import torch

from tests import shapes as S


def _kernel_case_names():
    """{kernel instantiation: first parity case that runs it} over the kernel-level cases of tests/test_kernels_gpu.py."""
    from x3d_tf_amd import hip
    got = {}

    def add(st, what):
        got.setdefault(hip.kernel_name(st), what)

    for dt in S.DTYPES:
        half = dt != S.F32
        for shp in S.PW_FWD + S.PW_FWD_XL:
            add(S.pw_fwd_struct(shp, dt, False), f"test_pw_fwd[{shp}, {dt}]")
            if half:
                add(S.pw_fwd_struct(shp, dt, True), f"test_pw_fwd[{shp}, {dt}, panel]")
        for shp in S.PW_FWD_TAIL:
            add(S.pw_fwd_struct(shp, dt, False), f"test_pw_fwd_tail[{shp}, {dt}]")
            if half:
                add(S.pw_fwd_struct(shp, dt, True), f"test_pw_fwd_tail[{shp}, {dt}, panel]")
        for shp in S.PW_FWD_INFER:
            add(S.pw_fwd_infer_struct(shp, dt, False), f"test_pw_fwd_infer[{shp}, {dt}]")
            if half:
                add(S.pw_fwd_infer_struct(shp, dt, True), f"test_pw_fwd_infer[{shp}, {dt}, panel]")
        for shp in S.PW_DGRAD:
            for epi in S.PW_DGRAD_EPI:
                add(S.pw_dgrad_struct(shp, epi, dt, False), f"test_pw_dgrad[{shp}, {epi}, {dt}]")
                if half:
                    add(S.pw_dgrad_struct(shp, epi, dt, True), f"test_pw_dgrad[{shp}, {epi}, {dt}, panel]")
        for shp in S.PW_WGRAD:
            add(S.pw_wgrad_struct(shp, dt), f"test_pw_wgrad[{shp}, {dt}]")
        if not half:
            for case in S.PW_F32_FULL:
                add(S.pw_f32_full_struct(case), f"test_pw_f32_past_buffer_offsets_fp64[{case}]")
        if half:
            for shp in S.PW_BWD:
                st = S.pw_bwd_struct(shp, dt)
                assert hip.load().x3d_pw_bwd_supported(st), f"fused backward does not cover the registered case {shp}"
                add(st, f"test_pw_bwd_oracle[{shp}, {dt}]")
            for shp in S.PW_BWD_TAIL:
                st = S.pw_bwd_struct(shp, dt)
                assert hip.load().x3d_pw_bwd_supported(st), f"fused backward with the tail does not cover the registered case {shp}"
                add(st, f"test_pw_bwd_tail[{shp}, {dt}]")
            for shp in S.PW_BWD_RC:
                st = S.pw_bwd_rc_struct(shp, dt)
                assert hip.load().x3d_pw_bwd_supported(st), f"the recomputed-output fused backward does not cover the registered case {shp}"
                add(st, f"test_pw_bwd_rc[{shp}, {dt}]")
            for shp in S.PW_BWD_RC_STRIDED:
                st = S.pw_bwd_rc_strided_struct(shp, dt)
                assert hip.load().x3d_pw_bwd_supported(st), f"the strided recomputed-output backward does not cover the registered case {shp}"
                add(st, f"test_pw_bwd_rc_strided[{shp}, {dt}]")
                # ... which also runs the DENSE store form on the even-pixel copy (the plans' path since round 6)
                n_, ci_, co_, t_, xh_, xw_ = shp
                st = S.pw_bwd_rc_struct((n_, ci_, co_, t_, (xh_ + 1) // 2, (xw_ + 1) // 2, "store", 0), dt)
                if hip.load().x3d_pw_bwd_supported(st):
                    add(st, f"test_pw_bwd_rc_strided[{shp}, {dt}, compact]")
        for shp in S.DW:
            add(S.dw_fwd_struct(shp, dt), f"test_dw3d_fwd[{shp}, {dt}]")
            add(S.dw_bwd_struct(shp, dt), f"test_dw3d_bwd[{shp}, {dt}]")
    return got


@pytest.fixture(scope="module")
def parity_kernels():
    # kernel-level cases only: the whole-model parity tests (tests/test_model_gpu.py) run the same instantiations again
    # inside full plans, but coverage is not allowed to lean on them
    return _kernel_case_names()


@pytest.mark.parametrize("index", [1, 2, 3, 4, 5])
def test_every_instantiation_of_a_baseline_config_has_a_parity_case(parity_kernels, index):
    from x3d_tf_amd import dispatch as D
    rows = D.baseline_kernels(index)
    assert rows, "the dry plan recorded no conv launches"
    need = D.kernel_set(rows)
    missing = {k: v for k, v in need.items() if k not in parity_kernels}
    assert not missing, (f"BASELINE config {index} {D.BASELINE_CONFIGS[index][:5]} dispatches kernel instantiations that no "
                         f"-m gpu oracle-parity case runs:\n" + "\n".join(f"  {k}   <- {v}" for k, v in sorted(missing.items())))


# ---- the shipped configurations (configs/kinetics/*.yaml) beyond the five BASELINE plans: every storage type, the yaml's global
# training batch on 1, 2, 4 and 8 GPUs, inference on one video (views x crops clips) and on TEST.BATCH_SIZE videos; clip length
# and crop from the yaml
SHIPPED_VARIANTS = ("XS", "S", "M", "L", "XL")


@functools.lru_cache(maxsize=None)
def shipped_config_plans(variant):
    """[(clips per GPU, T, crop, training)] of a shipped yaml."""
    import x3d_tf_amd as x
    cfg = x.get_config(variant)
    t, views = cfg.DATA.TEMP_DURATION, cfg.TEST.NUM_TEMPORAL_VIEWS * cfg.TEST.NUM_SPATIAL_CROPS
    return ([(cfg.TRAIN.BATCH_SIZE // d, t, cfg.DATA.TRAIN_CROP_SIZE, True) for d in (1, 2, 4, 8)]
            + [(views, t, cfg.DATA.TEST_CROP_SIZE, False), (cfg.TEST.BATCH_SIZE * views, t, cfg.DATA.TEST_CROP_SIZE, False)])


@functools.lru_cache(maxsize=None)
def shipped_config_kernels(variant=None, dtype=None):
    """{(entry point, instantiation): first launch that dispatches it} over the dry plans of a shipped yaml in one storage type
    (variant None: over all of them, every storage type)."""
    from x3d_tf_amd import dispatch as D
    got = {}
    if variant is None:
        for v in SHIPPED_VARIANTS:
            for dt in S.DTYPES:
                for k, what in shipped_config_kernels(v, dt).items():
                    got.setdefault(k, what)
        return got
    for n, t, s, training in shipped_config_plans(variant):
        for entry, kern, shape in D.config_kernels(variant, n, t, s, dtype, training):
            got.setdefault((entry, kern), f"X3D-{variant} {str(dtype)[6:]} {'training' if training else 'inference'}, {n} clips: {shape}")
    return got


@pytest.mark.parametrize("dtype", S.DTYPES, ids=lambda d: str(d)[6:])
@pytest.mark.parametrize("variant", SHIPPED_VARIANTS)
def test_every_instantiation_of_a_shipped_config_is_covered(parity_kernels, variant, dtype):
    """Every conv instantiation a shipped yaml dispatches -- training at its global batch on 1, 2, 4, 8 GPUs, inference on one
    video and on TEST.BATCH_SIZE videos -- is run by a registered kernel-level case, or is a class of the fused pointwise
    backward sweep (tests/pw_bwd_classes.py) or of the depthwise sweep (tests/dw_classes.py)."""
    from tests import dw_classes as DC
    from tests import pw_bwd_classes as PC
    need = shipped_config_kernels(variant, dtype)
    assert need, "the dry plans recorded no conv launches"
    pw_bwd, dw = PC.enumerate_classes(), DC.enumerate_classes()
    missing = {k: v for k, v in need.items()
               if k[1] not in parity_kernels and not (k[0] == "x3d_pw_bwd" and k[1] in pw_bwd) and k not in dw}
    assert not missing, (f"X3D-{variant} ({dtype}) dispatches kernel instantiations that no -m gpu parity case runs:\n"
                         + "\n".join(f"  {k[0]} {k[1]}   <- {v}" for k, v in sorted(missing.items())))


def test_bench_workload_is_config_3(parity_kernels):
    """bench.py's default workload (X3D-M, 64 clips of 16x224x224, bf16) is BASELINE config 3: the depthwise kernels of its
    216-channel 28 -> 14 layer (the pair VERDICT r01 found untested) are among the parity-tested instantiations by name."""
    from x3d_tf_amd import dispatch as D
    rows = [r for r in D.baseline_kernels(3) if r[0].startswith("x3d_dw3d") and r[2] == "N64 C216 T16 28x28 s2"]
    assert {r[0] for r in rows} == {"x3d_dw3d_fwd", "x3d_dw3d_bwd"}
    for _, kernel, _ in rows:
        assert kernel in parity_kernels, kernel


def test_dry_model_cannot_run():
    """A dry model records launches and nothing else: there is no CPU execution path."""
    import x3d_tf_amd as x
    from x3d_tf_amd import hip
    from x3d_tf_amd.model import X3D
    m = X3D(x.get_config("XS"), dtype=torch.float32, device="dry")
    with pytest.raises(hip.X3DHipError):
        m(torch.zeros(10, 4, 32, 32, 3), training=False)
    pl = m._plan(2, 4, 32, 32, True)
    with pytest.raises(hip.X3DHipError):
        pl.run(pl.fwd)


@pytest.mark.parametrize("index", [1, 5])
def test_inference_plan_is_inference_shaped(index):
    """BASELINE configs 1 and 5 (eval.py:83-89, model.py:113-127 at training=False): the recorded forward list has no
    residual-tail pass, no per-layer BatchNorm launch (one batched coefficient launch at the head) and per block exactly
    a -> b -> [SE] -> [shortcut conv] -> c, the last with the folded BN + Add + ReLU epilogue."""
    import x3d_tf_amd as x
    from x3d_tf_amd import dispatch as D
    from x3d_tf_amd.model import X3D
    variant, n, t, s, dtype, training, over = D.BASELINE_CONFIGS[index]
    flat = []
    for k, v in over.items():
        flat += [k, v]
    m = X3D(x.get_config(variant, flat or None), dtype=dtype, device="dry")
    pl = m._plan(n, t, s, s, training)
    names = [item[0] for item in pl.fwd]
    assert names[0] == "x3d_bn_eval_coef_batched" and names.count("x3d_bn_eval_coef_batched") == 1
    assert not [k for k in names if k.startswith(("x3d_tail", "x3d_bn_finalize"))]
    # the stem: one launch (conv_s -> conv_t -> BN + ReLU, x3d_stem_fwd) with 16-bit storage, the two-kernel path in fp32
    assert pl.stem_fused == (dtype != torch.float32)
    stem = ["x3d_stem_fwd"] if pl.stem_fused else ["x3d_stem_s_fwd", "x3d_dwt_fwd"]
    k0 = 1 + len(stem)
    assert names[1:k0] == stem
    blocks = m.arch.blocks
    odd_rows = lambda b: (pl.blocks[blocks.index(b)].wo % 2) == 1      # (only where the gather takes one output per load)
    want = []
    for b in blocks:
        # (a strided shortcut conv reads the even-pixel copy of the block input: one small copy launch in front of it)
        want += ["x3d_pw_fwd", "x3d_dw3d_fwd"] + (["x3d_se_fwd"] if b.has_se else []) + \
                ((["x3d_subsample2"] if b.stride == 2 and odd_rows(b) else []) + ["x3d_pw_fwd"] if b.has_shortcut_conv else []) + ["x3d_pw_fwd"]
    assert names[k0:k0 + len(want)] == want
    assert names[k0 + len(want):] == ["x3d_pw_fwd", "x3d_pool_fwd", "x3d_dense_fwd", "x3d_dense_fwd", "x3d_softmax_xent", "x3d_view_mean"]
    assert len(want) <= 6 * len(blocks) and sum(3 + b.has_se + b.has_shortcut_conv * (1 + (b.stride == 2 and odd_rows(b))) for b in blocks) == len(want)
    for B in pl.blocks:                      # the `c` conv carries the epilogue; `a` and the shortcut stay raw
        assert B.sc.out_scale_shift and B.sc.out_add and B.sc.out_act == 1 and not B.sc.stats
        assert bool(B.sc.out_add_scale_shift) == bool(B.spec.has_shortcut_conv)
        assert not B.sa.out_scale_shift
    # activation buffers are shared between blocks: two block outputs ping-pong
    ys = {B.y.data_ptr() for B in pl.blocks}
    assert len(ys) == 2 and len({B.a_raw.data_ptr() for B in pl.blocks}) == 1
    for prev, cur in zip(pl.blocks, pl.blocks[1:]):
        assert cur.x.data_ptr() == prev.y.data_ptr() and cur.y.data_ptr() != cur.x.data_ptr()



# the plans whose depthwise launches tests/test_full_size_gpu.py checks against fp64 at their real size (shapes.DW_FULL):
# BASELINE configs 2 - 5 and config 3 with fp16 storage (bench.py --dtype fp16)
DW_FULL_PLANS = {"2": 2, "3": 3, "3-fp16": ("M", 64, 16, 224, torch.float16, True), "4": 4, "5": 5}


def _dw_launches(plan):
    """(entry, kernel instantiation, argument struct) of every x3d_dw3d_fwd / x3d_dw3d_bwd launch of a full-size dry plan."""
    from x3d_tf_amd import hip
    from x3d_tf_amd.config import get_config
    from x3d_tf_amd.dispatch import BASELINE_CONFIGS
    from x3d_tf_amd.model import X3D
    variant, n, t, s, dtype, training, over = BASELINE_CONFIGS[plan] if isinstance(plan, int) else plan + ({},)
    flat = [x for kv in over.items() for x in kv]
    m = X3D(get_config(variant, flat or None), dtype=dtype, device="dry")
    pl = m._plan(n, t, s, s, training)
    out = []
    for lst in (pl.fwd, pl.bwd):
        for i, item in enumerate(lst):
            if item is not None and item[0] in ("x3d_dw3d_fwd", "x3d_dw3d_bwd"):
                st = pl.structs[(id(lst), i)]
                out.append((item[0], hip.kernel_name(st), st))
    m.release_plans()
    return out


def _dw_launch_key(entry, st):
    """shapes.DW_FULL's key (entry, dtype, N, C, T, H, W, stride, prologue, stats, pool) of a recorded depthwise launch."""
    from x3d_tf_amd import hip
    dtype = [d for d in S.DTYPES if hip.dtype_code(d) == st.dtype][0]
    head = ("fwd" if entry == "x3d_dw3d_fwd" else "bwd", dtype, st.N, st.C, st.T, st.H, st.W, st.stride)
    if entry == "x3d_dw3d_bwd":
        return head + (None, None, None)
    return head + ("bn" if st.in_bn else "ss", bool(st.stats), bool(st.pool))


def _dw_full_cover(launches):
    """{launch key: message} of the launches without a full-size fp64 case.  A forward launch is covered by the DW_FULL entry
    of its own key, or by the entry of its shape and prologue with the OTHER pool / stats setting if both dispatch the same
    kernel instantiation (asserted here through hip.kernel_name, not assumed); a case must run the plan's kernel."""
    from x3d_tf_amd import hip
    cases = set(S.DW_FULL)
    missing = {}
    for entry, kern, st in launches:
        key = _dw_launch_key(entry, st)
        alts = [key] if key[0] == "bwd" else [key[:9] + (sts, pool) for sts in (key[9], not key[9]) for pool in (key[10], not key[10])]
        got = [a for a in alts if a in cases]
        why = "no DW_FULL entry of this shape and form"
        for a in got:
            case_kern = hip.kernel_name(S.dw_full_struct(a))
            if case_kern == kern:
                break
            why = f"the DW_FULL case {S.dw_full_id(a)} runs {case_kern}"
        else:
            missing[key] = f"{S.dw_full_id(key)} ({kern}): {why}"
    return missing


@pytest.mark.parametrize("plan", list(DW_FULL_PLANS))
def test_every_depthwise_launch_of_a_full_size_plan_has_a_full_size_case(plan):
    """Every x3d_dw3d_fwd / x3d_dw3d_bwd launch of the plan has a shapes.DW_FULL case (tests/test_full_size_gpu.py:
    test_depthwise_full_size) at its real size and in its launch form, which dispatches the same kernel as the plan."""
    launches = _dw_launches(DW_FULL_PLANS[plan])
    assert launches, "the dry plan recorded no depthwise launches"
    missing = _dw_full_cover(launches)
    assert not missing, (f"plan {plan}: depthwise launches without a full-size fp64 case (tests/shapes.py DW_FULL):\n"
                         + "\n".join(f"  {v}" for v in sorted(set(missing.values()))))


def test_every_dw_full_case_is_a_launch_of_a_full_size_plan():
    """... and no DW_FULL case is left over from a plan that no longer launches it (a case that stands for a launch form
    only through the kernel-sameness rule still has the shape of a real launch)."""
    keys = {_dw_launch_key(e, st)[:9] for plan in DW_FULL_PLANS.values() for e, _, st in _dw_launches(plan)}
    stale = [S.dw_full_id(c) for c in S.DW_FULL if c[:9] not in keys]
    assert not stale, "DW_FULL cases that no full-size plan launches: " + ", ".join(stale)


# ---- the pointwise launches of the same plans (shapes.PW_FULL; tests/test_full_size_gpu.py: test_pointwise_full_size) ----
PW_FULL_PLANS = DW_FULL_PLANS
_PW_ENTRIES = {"x3d_pw_fwd": "fwd", "x3d_pw_dgrad": "dgrad", "x3d_pw_wgrad": "wgrad", "x3d_pw_bwd": "bwd"}


def _pw_launches(plan):
    """(entry, kernel instantiation, argument struct) of every pointwise launch of a full-size dry plan."""
    from x3d_tf_amd import hip
    from x3d_tf_amd.config import get_config
    from x3d_tf_amd.dispatch import BASELINE_CONFIGS
    from x3d_tf_amd.model import X3D
    variant, n, t, s, dtype, training, over = BASELINE_CONFIGS[plan] if isinstance(plan, int) else plan + ({},)
    flat = [x for kv in over.items() for x in kv]
    m = X3D(get_config(variant, flat or None), dtype=dtype, device="dry")
    pl = m._plan(n, t, s, s, training)
    out = []
    for lst in (pl.fwd, pl.bwd):
        for i, item in enumerate(lst):
            if item is not None and item[0] in _PW_ENTRIES:
                st = pl.structs[(id(lst), i)]
                out.append((item[0], hip.kernel_name(st), st, _pw_launch_key(item[0], st)))   # (while the plan holds its folds)
    m.release_plans()
    return out


def _pw_launch_key(entry, st):
    """shapes.PW_FULL's key of a recorded pointwise launch (shapes.py documents the fields)."""
    from x3d_tf_amd import hip
    e = _PW_ENTRIES[entry]
    dtype = [d for d in S.DTYPES if hip.dtype_code(d) == st.dtype][0]
    v = lambda k: bool(getattr(st, k, None))
    if e == "fwd":
        flags = dict(stats=v("stats"), ss=v("in_scale_shift"), gate=v("in_gate"), add=v("in_add"), add_ss=v("in_add_scale_shift"),
                     store=v("in_store"), oss=v("out_scale_shift"), oadd=v("out_add"), oadd_ss=v("out_add_scale_shift"))
        mode = (st.stride, None, st.in_act, st.out_act)
    elif e == "wgrad":
        flags = dict(ss=v("in_scale_shift"), gate=v("in_gate"), slab=v("dw_slab"), fold=v("coef_fold"))
        mode = (st.stride, None, st.in_act, None)
    else:
        fold = hip.FOLDS.get(st.coef_fold) if st.coef_fold else None
        assert not st.coef_fold or fold is not None, "a coef_fold address that hip.FOLDS does not know"
        flags = dict(gate=v("gate"), tail_c=v("tail_c"), tail_r=v("tail_r"), rc=v("rc_panel"), slab=v("dw_slab"),
                     fold=fold is not None, pub=fold is not None and bool(fold.dgamma))
        mode = (st.x_stride if e == "bwd" else None, st.epi, None, None)
    h, w = (st.xH, st.xW) if e == "bwd" and st.x_stride == 2 else (st.H, st.W)
    return (e, dtype, st.N, st.Cin, st.Cout, st.T, h, w) + mode + (tuple(f for f in S.PW_FLAGS if flags.get(f)),)


def _pw_alts(key):
    """The PW_FULL keys that may stand for a launch of this key: itself, and the same shape and form with the SE gate and / or
    the fold's publishing added (the coverage test then requires that they dispatch the same kernel)."""
    form = set(key[12])
    extra = [set()] + [{"gate"}] + ([{"pub"}, {"gate", "pub"}] if "fold" in form else [])
    out = []
    for x in extra:
        alt = key[:12] + (tuple(f for f in S.PW_FLAGS if f in form | x),)
        if alt not in out:
            out.append(alt)
    return out


@pytest.fixture(scope="module")
def pw_plan_launches():
    return {plan: _pw_launches(p) for plan, p in PW_FULL_PLANS.items()}


def _pw_full_cover(launches):
    """{launch key: message} of the launches without a full-size fp64 case that dispatches the plan's kernel."""
    from x3d_tf_amd import hip
    cases = set(S.PW_FULL)
    missing = {}
    for entry, kern, st, key in launches:
        why = "no PW_FULL entry of this shape and form"
        for a in [a for a in _pw_alts(key) if a in cases]:
            case_kern = hip.kernel_name(S.pw_full_struct(a))
            if case_kern == kern:
                break
            why = f"the PW_FULL case {S.pw_full_id(a)} runs {case_kern}"
        else:
            missing[key] = f"{S.pw_full_id(key)} ({kern}): {why}"
    return missing


@pytest.mark.parametrize("plan", list(PW_FULL_PLANS))
def test_every_pointwise_launch_of_a_full_size_plan_has_a_full_size_case(pw_plan_launches, plan):
    """Every x3d_pw_fwd / _dgrad / _wgrad / _bwd launch of the plan has a shapes.PW_FULL case (tests/test_full_size_gpu.py:
    test_pointwise_full_size) at its real size and in its launch form, which dispatches the same kernel as the plan; and every
    slab-form launch sizes its slabs as the case's struct does (x3d_pw_bwd_dw_parts / x3d_pw_wgrad_dw_parts)."""
    import ctypes as C
    from x3d_tf_amd import hip
    launches = pw_plan_launches[plan]
    assert launches, "the dry plan recorded no pointwise launches"
    missing = _pw_full_cover(launches)
    assert not missing, (f"plan {plan}: pointwise launches without a full-size fp64 case (tests/shapes.py PW_FULL):\n"
                         + "\n".join(f"  {v}" for v in sorted(set(missing.values()))))
    cases = set(S.PW_FULL)
    for entry, _, st, key in launches:
        if getattr(st, "dw_slab", None):
            case = [a for a in _pw_alts(key) if a in cases][0]
            query = hip.load().x3d_pw_wgrad_dw_parts if entry == "x3d_pw_wgrad" else hip.load().x3d_pw_bwd_dw_parts
            cs = S.pw_full_struct(case)
            assert st.dw_slab_parts == cs.dw_slab_parts == query(C.byref(cs)) > 0, S.pw_full_id(key)


def test_every_pw_full_case_is_a_launch_of_a_full_size_plan(pw_plan_launches):
    """... and no PW_FULL case is left over: each one is a launch key of a plan, or stands for one by the gate / publishing
    rule."""
    keys = {a for ls in pw_plan_launches.values() for _, _, _, key in ls for a in _pw_alts(key)}
    stale = [S.pw_full_id(c) for c in S.PW_FULL if c not in keys]
    assert not stale, "PW_FULL cases that no full-size plan launches: " + ", ".join(stale)
    assert len(set(S.PW_FULL)) == len(S.PW_FULL), "duplicate PW_FULL entries"


# ---- every other launch of the same plans (shapes.AUX_FULL; tests/test_full_size_gpu.py: test_aux_full_size) ---------------
AUX_FULL_PLANS = DW_FULL_PLANS
# covered elsewhere: the pointwise and depthwise lists above, the stem's full-size tests, and the side-stream join (no kernel)
_AUX_ELSEWHERE = ("x3d_pw_fwd", "x3d_pw_dgrad", "x3d_pw_wgrad", "x3d_pw_bwd", "x3d_dw3d_fwd", "x3d_dw3d_bwd", "x3d_stem_fwd",
                  "x3d_stem_bwd", "x3d_stem_s_fwd", "x3d_stem_s_wgrad", "x3d_dwt_fwd", "x3d_dwt_bwd", "side_join")


def _dtype_of(code):
    from x3d_tf_amd import hip
    return [d for d in S.DTYPES if hip.dtype_code(d) == code][0]


def _nz(p):
    return bool(p)


# one key extractor per entry name, over the recorded argument tuple `a` (C ABI order, the stream excluded), the plan and
# the launch's argument struct; shapes.py documents the fields
_AUX_KEYS = {
    "x3d_tail_bwd": lambda a, pl, st: ("tail_bwd", _dtype_of(a[9]), a[6], a[7], a[8], _nz(a[3])),
    "x3d_relu_bn_bwd_reduce": lambda a, pl, st: ("relu_bn_bwd_reduce", _dtype_of(a[9]), a[6], a[7], a[8],
                                                 "dy" if _nz(a[0]) else "dpool", _nz(a[4])),
    "x3d_pool_fwd": lambda a, pl, st: ("pool_fwd", _dtype_of(a[6]), a[3], a[4], a[5]),
    "x3d_subsample2": lambda a, pl, st: ("subsample2", _dtype_of(a[5]), a[2], a[3], a[4]),
    "x3d_se_fwd": lambda a, pl, st: ("se_fwd", a[9], a[10], a[11], int(a[1])),
    "x3d_se_bnb_bwd": lambda a, pl, st: ("se_bnb_bwd", st.N, st.C, st.Wd, int(st.P), bool(st.w1),
                                         tuple((j.parts, j.elems) for j in st.reduce if j.slab)),
    "x3d_dense_fwd": lambda a, pl, st: ("dense_fwd", a[7], a[8], a[9], a[6], a[2] if _nz(a[1]) else None, _nz(a[4])),
    "x3d_dense_bwd": lambda a, pl, st: ("dense_bwd", a[10], a[11], a[12], a[2], a[5] if _nz(a[4]) else None, _nz(a[7]),
                                        _nz(a[9])),
    "x3d_softmax_xent": lambda a, pl, st: ("softmax_xent", a[6], a[7], a[5], _nz(a[1])),
    "x3d_view_mean": lambda a, pl, st: ("view_mean", a[2], a[3], a[4]),
    "x3d_bn_finalize": lambda a, pl, st: ("bn_finalize", a[11], int(a[1]), a[8]),
    "x3d_bn_bwd_finalize": lambda a, pl, st: ("bn_bwd_finalize", a[7], int(a[1])),
    "x3d_bn_bwd_finalize_rc": lambda a, pl, st: ("bn_bwd_finalize_rc", _dtype_of(a[18]), a[7], int(a[1]), a[11],
                                                 (a[16], a[17]) if _nz(a[12]) else None),
    "x3d_bn_eval_coef_batched": lambda a, pl, st: ("bn_eval_coef_batched", tuple(it.C for it in pl.bn_eval_items)),
}
# standalone halves of the recomputed-output backward: covered by a PW_FULL `rc` case of the same (Cout, Cin, dtype), which
# runs both at full size through ops.pw_bwd_rc
_AUX_RC = {"x3d_pw_bwd_rc_prepare": lambda a: (a[4], a[5], _dtype_of(a[6])),
           "x3d_pw_bwd_rc_finish": lambda a: (a[4], a[5], _dtype_of(a[6]))}


def _aux_launches(plan):
    """(entry, key) of every launch of a full-size dry plan that the pointwise / depthwise / stem lists do not cover; an
    entry name this file does not know fails here (a new launch needs a key and a full-size case)."""
    from x3d_tf_amd.config import get_config
    from x3d_tf_amd.dispatch import BASELINE_CONFIGS
    from x3d_tf_amd.model import X3D
    variant, n, t, s, dtype, training, over = BASELINE_CONFIGS[plan] if isinstance(plan, int) else plan + ({},)
    flat = [x for kv in over.items() for x in kv]
    m = X3D(get_config(variant, flat or None), dtype=dtype, device="dry")
    pl = m._plan(n, t, s, s, training)
    out, unknown = [], set()
    for lst in (pl.fwd, pl.bwd):
        for i, item in enumerate(lst):
            if item is None or item[0] in _AUX_ELSEWHERE:
                continue
            name, args = item[0], item[2]
            if name in _AUX_RC:
                out.append((name, ("rc",) + _AUX_RC[name](args)))
            elif name in _AUX_KEYS:
                out.append((name, _AUX_KEYS[name](args, pl, pl.structs.get((id(lst), i)))))
            else:
                unknown.add(name)
    m.release_plans()
    assert not unknown, f"launches tests/test_dispatch_coverage.py has no AUX_FULL key for: {sorted(unknown)}"
    return out


@pytest.fixture(scope="module")
def aux_plan_launches():
    return {plan: _aux_launches(p) for plan, p in AUX_FULL_PLANS.items()}


def _pw_rc_cases():
    return {(co, ci, dt) for (e, dt, n, ci, co, *_r, form) in S.PW_FULL if e == "bwd" and "rc" in form}


@pytest.mark.parametrize("plan", list(AUX_FULL_PLANS))
def test_every_aux_launch_of_a_full_size_plan_has_a_full_size_case(aux_plan_launches, plan):
    """Every launch of the plan outside the pointwise, depthwise and stem families (BatchNorm bookkeeping, residual-tail
    backward, squeeze-excite, slab reductions, head, loss) has a shapes.AUX_FULL case at its real size and in its launch form;
    a standalone x3d_pw_bwd_rc_prepare / _finish has a PW_FULL `rc` case of its (Cout, Cin, dtype)."""
    launches = aux_plan_launches[plan]
    assert launches, "the dry plan recorded no other launches"
    cases, rc = set(S.AUX_FULL), _pw_rc_cases()
    missing = sorted({f"{e}: {key[1:] if key[0] == 'rc' else S.aux_full_id(key)}" for e, key in launches
                      if (key[1:] not in rc if key[0] == "rc" else key not in cases)})
    assert not missing, (f"plan {plan}: launches without a full-size fp64 case (tests/shapes.py AUX_FULL):\n"
                         + "\n".join(f"  {v}" for v in missing))


def test_every_aux_full_case_is_a_launch_of_a_full_size_plan(aux_plan_launches):
    """... and no AUX_FULL case is left over from a plan that no longer launches it, nor listed twice."""
    keys = {key for ls in aux_plan_launches.values() for _, key in ls}
    stale = [S.aux_full_id(c) for c in S.AUX_FULL if c not in keys]
    assert not stale, "AUX_FULL cases that no full-size plan launches: " + ", ".join(stale)
    assert len(set(S.AUX_FULL)) == len(S.AUX_FULL), "duplicate AUX_FULL entries"
