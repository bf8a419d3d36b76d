"""ctypes binding of libx3d_hip.so (C ABI in include/x3d_hip.h).

There is no fallback: if the library is missing or a call fails this raises.  torch is used only for
device memory (``tensor.data_ptr()``) and the current HIP stream.
"""
import ctypes as C
import os
import re
import weakref

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("X3D_HIP_LIB") or os.path.join(_HERE, "libx3d_hip.so")   # X3D_HIP_LIB: A/B builds (tools/build_variant.sh)

_vp, _i, _f, _d, _ll = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_longlong


class X3DHipError(RuntimeError):
    pass


# ---- include/x3d_hip.h is the single statement of the ABI: constants, argument structs and signatures are read from it ----
_SCALARS = {"int": _i, "float": _f, "double": _d, "long long": _ll, "unsigned short": C.c_ushort,
            "size_t": C.c_size_t, "uint32_t": C.c_uint32}
_POINTEES = set(_SCALARS) | {"void", "unsigned char"}   # data pointers: callers hand over integers from data_ptr() -> c_void_p
# Where Python passes a host object instead of an address the header cannot say so.  (struct or function, field or parameter)
# -> ctypes type, or the name of a header struct for a pointer to it.  A pointer to a header struct in a PARAMETER is
# POINTER(struct) by default (callers pass byref(args)); inside a struct it is an address held as an integer (coef_fold via
# fold_address(), which dispatch._struct_pointers follows; JpegDecodeArgs.images / host_images).
_OVERRIDES = {
    ("x3d_dw3d_fwd_args", "in_bn"): "x3d_bn_fold",                  # plan.py assigns ctypes.pointer(BnFold) to the field
    ("x3d_bn_eval_coef_batched", "items"): _vp,                     # the item table lives in device memory: data_ptr()
    ("x3d_pw_pack_weights", "items"): _vp,                          # likewise
    ("x3d_crc32c", "data"): C.c_char_p,                             # callers pass bytes
    ("x3d_train_resized_hw", "new_h"): C.POINTER(_i),               # host out-parameters: byref(c_int())
    ("x3d_train_resized_hw", "new_w"): C.POINTER(_i),
    ("x3d_jpeg_parse", "scratch_bytes"): C.POINTER(_ll),            # host out-parameter: byref(c_longlong())
    ("x3d_train_clips_aug", "mean"): C.POINTER(_f),                 # host float[3]: callers pass a ctypes array
    ("x3d_train_clips_aug", "std"): C.POINTER(_f),
}
_ITEM = re.compile(r"(?:((?:\w+[\s*]+)+))?(\w+)((?:\[\d+\])*)$")    # [type] name [dims]: `const float* w`, `Cin`, `qt[3][64]`
_DECL = re.compile(r"(?:typedef\s+struct\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>x3d_\w+)"
                   r"|(?P<ret>[\w\s*]+?)(?P<fn>x3d_\w+)\s*\((?P<params>[^(){};]*)\))\s*;\s*")


def _parse_header(text, overrides=_OVERRIDES):
    """(constants, structs, signatures) of a header in the style of include/x3d_hip.h; a declaration this does not understand
    raises X3DHipError naming its line."""
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)   # line numbers survive
    consts, structs, sigs = {}, {}, {}

    def fail(pos, why):
        decl = " ".join(text[pos:].split(";")[0].split())
        raise X3DHipError(f"x3d_hip.h line {text.count(chr(10), 0, pos) + 1}: {why}: `{decl[:120]}`")

    def ctype(pos, owner, ty, name, param):
        words = ty.replace("*", " ").split()
        base, stars = " ".join(w for w in words if w != "const"), ty.count("*")
        over = overrides.get((owner, name))
        if over is not None:
            return C.POINTER(structs[over]) if isinstance(over, str) else over
        if not stars and (base in _SCALARS or base in structs):
            return _SCALARS.get(base) or structs[base]
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and base in structs and param:
            return C.POINTER(structs[base])
        if stars and (base in _POINTEES or base in structs):
            return _vp
        fail(pos, f"unknown type `{ty.strip()}` of `{name}`")

    def items(pos, owner, decl, param):
        """`int N, Cin` / `float mean[3]` / `const void* x` -> [(name, ctype)]"""
        out, ty = [], None
        for part in decl.split(","):
            m = _ITEM.match(part.strip())
            if not m or not (m.group(1) or ty) or (m.group(1) and out) or (out and "*" in ty):
                fail(pos, "cannot read declaration")
            ty = m.group(1) or ty
            ct = ctype(pos, owner, ty, m.group(2), param)
            for n in reversed(re.findall(r"\d+", m.group(3))):
                ct = ct * int(n)
            out.append((m.group(2), ct))
        return out

    def directive(m):
        d = re.fullmatch(r"#\s*define\s+X3D_(\w+)\s+(-?\d+)\s*", m.group())
        if d:
            consts[d.group(1)] = int(d.group(2))
        elif not re.match(r"#\s*(ifn?def|endif|include|define\s+\w+\s*$)", m.group()):
            fail(m.start(), "cannot read directive")
        return ""
    text = re.sub(r"^[ \t]*#.*$", directive, text, flags=re.M)
    text = re.sub(r'^(extern "C" \{|\})[ \t]*$', "", text, flags=re.M)
    pos = re.match(r"\s*", text).end()
    while pos < len(text):
        m = _DECL.match(text, pos) or fail(pos, "cannot read declaration")
        if m.group("struct"):
            fields, end = [], 0
            for d in re.finditer(r"\s*([^;]+);", m.group("body")):
                fields += items(m.start("body") + d.start(1), m.group("struct"), d.group(1), False)
                end = d.end()
            if m.group("body")[end:].strip():
                fail(m.start("body") + end, "cannot read declaration")
            name = "".join(w.capitalize() for w in m.group("struct")[4:].split("_"))      # x3d_pw_fwd_args -> PwFwdArgs
            structs[m.group("struct")] = type(name, (C.Structure,), {"_fields_": fields})
        else:
            fn, params = m.group("fn"), m.group("params").strip()
            args = [] if params == "void" else [a for p in params.split(",") for a in items(pos, fn, p, True)]
            sigs[fn] = ([t for _, t in args], ctype(pos, fn, m.group("ret"), "(return value)", False))
        pos = m.end()
    return consts, structs, sigs


with open(os.path.join(os.path.dirname(_HERE), "include", "x3d_hip.h")) as _fh:
    _CONSTS, _STRUCTS, _SIGS = _parse_header(_fh.read())


def _consts(*names):
    return [_CONSTS[n] for n in names]


def _struct(cname, doc=None):
    _STRUCTS[cname].__doc__ = doc
    return _STRUCTS[cname]


# one line per exported name: a constant or struct the header renames fails here, at import
ABI_VERSION = _consts("ABI_VERSION")[0]   # load() refuses a library built from another version of the header
F32, BF16, F16 = _consts("F32", "BF16", "F16")
ACT_NONE, ACT_RELU, ACT_SWISH, ACT_SIGMOID = _consts("ACT_NONE", "ACT_RELU", "ACT_SWISH", "ACT_SIGMOID")
MIX_MIXUP, MIX_CUTMIX = _consts("MIX_MIXUP", "MIX_CUTMIX")
EPI_STORE, EPI_ADD, EPI_ADD_STRIDED, EPI_SWISH_BWD = _consts("EPI_STORE", "EPI_ADD", "EPI_ADD_STRIDED", "EPI_SWISH_BWD")
AP_MAX_POSITIVES = _consts("AP_MAX_POSITIVES")[0]
SEG_CHUNK = _consts("SEG_CHUNK")[0]         # elements per chunk of the layer-wise optimizers' chunk table (segments.py)
LOSS_SCALE_STATE = _consts("LOSS_SCALE_STATE")[0]   # doubles of the device loss-scaler state (ops.loss_scale_state)
AUG_CROP_JITTER, AUG_CROP_RRC, AUG_ERASE_CONST, AUG_ERASE_PIXEL = _consts("AUG_CROP_JITTER", "AUG_CROP_RRC", "AUG_ERASE_CONST",
                                                                          "AUG_ERASE_PIXEL")
AUG_MEAN_PARTS, AUG_GEOM_COLS, AUG_COLOR_COLS, AUG_C_K = _consts("AUG_MEAN_PARTS", "AUG_GEOM_COLS", "AUG_COLOR_COLS", "AUG_C_K")
# column -> index of the int32 geometry table of x3d_train_clips_aug: AUG_G["START"] ...
AUG_G = {n[6:]: v for n, v in _CONSTS.items() if n.startswith("AUG_G_")}
# RandAugment (x3d_randaug_clips): op name as aug.RandAugOp spells it -> X3D_RA_* code, and the table geometry views.py fills
RA_OPS = {name: _CONSTS["RA_" + const] for name, const in dict(
    none="NONE", AutoContrast="AUTOCONTRAST", Equalize="EQUALIZE", Invert="INVERT", Rotate="ROTATE", Posterize="POSTERIZE",
    Solarize="SOLARIZE", SolarizeAdd="SOLARIZE_ADD", Color="COLOR", Contrast="CONTRAST", Brightness="BRIGHTNESS",
    Sharpness="SHARPNESS", ShearX="SHEAR_X", ShearY="SHEAR_Y", TranslateXRel="TRANSLATE_X", TranslateYRel="TRANSLATE_Y",
    copy="COPY").items()}
RA_CLIP_COLS, RA_OP_COLS, RA_X_COLS, RA_FRAC_BITS = _consts("RA_CLIP_COLS", "RA_OP_COLS", "RA_X_COLS", "RA_FRAC_BITS")
RA_O_OP, RA_O_IARG, RA_O_FARG, RA_X_A, RA_X_SRC, RA_X_DST = _consts("RA_O_OP", "RA_O_IARG", "RA_O_FARG", "RA_X_A", "RA_X_SRC",
                                                                    "RA_X_DST")
# columns of the int64 layer table of x3d_precise_bn_accum / x3d_precise_bn_final (plan._Plan.precise_bn_table)
PBN_COLS, PBN_STATS, PBN_C, PBN_COUNT, PBN_MEAN, PBN_VAR, PBN_POOLED = _consts("PBN_COLS", "PBN_STATS", "PBN_C", "PBN_COUNT",
                                                                               "PBN_MEAN", "PBN_VAR", "PBN_POOLED")
JPEG_OK, JPEG_UNSUPPORTED, JPEG_MALFORMED, JPEG_CORRUPT, JPEG_SKIPPED = _consts(
    "JPEG_OK", "JPEG_UNSUPPORTED", "JPEG_MALFORMED", "JPEG_CORRUPT", "JPEG_SKIPPED")

PwFwdArgs = _struct("x3d_pw_fwd_args")
PwDgradArgs = _struct("x3d_pw_dgrad_args")
PwBwdArgs = _struct("x3d_pw_bwd_args")
DwReduceJob = _struct("x3d_dw_reduce_job")
EvalViewsArgs = _struct("x3d_eval_views_args")
TrainClipArgs = _struct("x3d_train_clip_args")
BnEvalItem = _struct("x3d_bn_eval_item")
PwPackItem = _struct("x3d_pw_pack_item")
PwWgradArgs = _struct("x3d_pw_wgrad_args")
BnBwdFold = _struct("x3d_bn_bwd_fold", "x3d_bn_bwd_fold: the BatchNorm-backward finalize folded into its consumers (coef_fold "
                    "of the backward argument structs).")
BnFold = _struct("x3d_bn_fold")
Dw3dFwdArgs = _struct("x3d_dw3d_fwd_args")
Dw3dBwdArgs = _struct("x3d_dw3d_bwd_args")
SeBnbBwdArgs = _struct("x3d_se_bnb_bwd_args")
JpegImage = _struct("x3d_jpeg_image", "x3d_jpeg_image: one parsed JPEG (include/x3d_hip.h).")
JpegDecodeArgs = _struct("x3d_jpeg_decode_args")

# address -> BnBwdFold: argument structs refer to a fold by address (tools that walk a plan's pointers follow it).  Weak values:
# the plan (or the ops wrapper) that built a fold keeps it alive for as long as its launches exist; an entry whose owner is gone
# disappears with it instead of accumulating -- and instead of handing dispatch._struct_pointers stale device addresses.
FOLDS = weakref.WeakValueDictionary()


def fold_address(f: BnBwdFold) -> int:
    """Address to put into an argument struct's `coef_fold`; the caller keeps `f` alive for as long as launches use it."""
    a = C.addressof(f)
    FOLDS[a] = f
    return a


_lib = None


def exported_symbols():
    """Names include/x3d_hip.h declares (and this binding expects)."""
    return sorted(_SIGS)


def load(path=None):
    """dlopen libx3d_hip.so and type every entry point.  Raises if it is missing."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise X3DHipError(
            f"{p} not found: build it with `python x3d-tf_amd/build.py` (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the X3D hot path.")
    lib = C.CDLL(p)
    lib.x3d_version.restype = _i
    have = int(lib.x3d_version())
    if have != ABI_VERSION:     # a stale .so (they ship out of band, git-ignored) would take shifted arguments silently
        raise X3DHipError(f"{p} has ABI version {have}, this binding needs {ABI_VERSION}: rebuild it "
                          "(`python x3d-tf_amd/build.py`)")
    for name, (argtypes, restype) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.argtypes = argtypes
        fn.restype = restype
    if path is None:
        _lib = lib
    return lib


def dilated(args, dilation):
    """`args` (a Dw3dFwdArgs / Dw3dBwdArgs) tagged with the dilation its launch passes to x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil.
    The C structs have no such field (the dilation is an argument of the dilated entry points): the tag is an attribute of
    the Python object, so that whoever holds the struct of a recorded launch -- dw3d_kernel_name, dispatch, the per-launch
    tools -- names and describes the launch that was recorded.  Returns args."""
    args.dilation = int(dilation)
    return args


def dw3d_dilation(args) -> int:
    """The dilation a depthwise argument struct was tagged with (dilated); 1 for an untagged one."""
    return int(getattr(args, "dilation", 1))


def dw3d_kernel_name(args):
    """Instantiation x3d_dw3d_fwd / x3d_dw3d_bwd -- or, for a struct tagged with a dilation >= 2 (dilated), x3d_dw3d_fwd_dil /
    x3d_dw3d_bwd_dil -- would launch for this argument struct (no launch)."""
    buf = C.create_string_buffer(128)
    fwd = C.byref(args) if isinstance(args, Dw3dFwdArgs) else None
    bwd = C.byref(args) if isinstance(args, Dw3dBwdArgs) else None
    d = dw3d_dilation(args)
    if d in (0, 1):
        rc = load().x3d_dw3d_kernel_name(fwd, bwd, buf, 128)
    else:
        rc = load().x3d_dw3d_kernel_name_dil(fwd, bwd, d, buf, 128)
    if rc != 0:
        raise X3DHipError(load().x3d_last_error().decode())
    return buf.value.decode()


def pw_kernel_name(args):
    """Instantiation x3d_pw_fwd / x3d_pw_dgrad / x3d_pw_wgrad / x3d_pw_bwd would launch for this argument struct (no
    launch, no GPU needed)."""
    buf = C.create_string_buffer(160)
    slots = [None, None, None, None]
    for i, kind in enumerate((PwFwdArgs, PwDgradArgs, PwWgradArgs, PwBwdArgs)):
        if isinstance(args, kind):
            slots[i] = C.byref(args)
    rc = load().x3d_pw_kernel_name(*slots, buf, 160)
    if rc != 0:
        raise X3DHipError(load().x3d_last_error().decode())
    return buf.value.decode()


STEM_ENTRIES = ("x3d_stem_s_fwd", "x3d_stem_s_wgrad", "x3d_dwt_fwd", "x3d_dwt_bwd", "x3d_stem_fwd", "x3d_stem_bwd")
STEM_NAME_STATS, STEM_NAME_OUT_SS, STEM_NAME_OUT_RELU, STEM_NAME_RELU_SS = _consts("STEM_NAME_STATS", "STEM_NAME_OUT_SS",
                                                                                   "STEM_NAME_OUT_RELU", "STEM_NAME_RELU_SS")


def stem_launch_query(entry, args):
    """The arguments of x3d_stem_kernel_name (without `out`, `cap`) for a launch of a stem entry point given by its own
    positional arguments `args` (C ABI order, the stream excluded: what a plan records): the tensor operands' addresses, the launch
    form as X3D_STEM_NAME_* flags, the extents."""
    a = list(args)
    nz = lambda p, flag: flag if p else 0
    if entry == "x3d_stem_s_fwd":          # x, w, y, N, Cin, T, H, W, Cout, dtype, x_layout
        ops_, flags, (n, cin, t, h, w, cout, dt, lay), kt = (a[0], a[2]), 0, a[3:11], 0
    elif entry == "x3d_stem_s_wgrad":      # x, dy, dw, N, Cin, T, H, W, Cout, dtype, x_layout
        ops_, flags, (n, cin, t, h, w, cout, dt, lay), kt = (a[0], a[1]), 0, a[3:11], 0
    elif entry == "x3d_dwt_fwd":           # x, w, y, stats, out_scale_shift, out_act, N, C, T, HW, KT, dtype
        ops_ = (a[0], a[2])
        flags = nz(a[3], STEM_NAME_STATS) | nz(a[4], STEM_NAME_OUT_SS) | nz(a[5] == ACT_RELU, STEM_NAME_OUT_RELU)
        (n, cout, t, hw, kt, dt), cin, h, w, lay = a[6:12], 0, 1, a[9], 0
    elif entry == "x3d_dwt_bwd":           # g, yraw, relu_scale_shift, coef, x, w, dx, dw, N, C, T, HW, KT, dtype
        ops_, flags = (a[0], a[1], a[4], a[6]), nz(a[2], STEM_NAME_RELU_SS)
        (n, cout, t, hw, kt, dt), cin, h, w, lay = a[8:14], 0, 1, a[11], 0
    elif entry == "x3d_stem_fwd":          # x, w_s, w_t, y, stats, out_scale_shift, out_act, N, Cin, T, H, W, Cout, KT, dtype, x_layout
        ops_ = (a[0], a[3])
        flags = nz(a[4], STEM_NAME_STATS) | nz(a[5], STEM_NAME_OUT_SS) | nz(a[6] == ACT_RELU, STEM_NAME_OUT_RELU)
        n, cin, t, h, w, cout, kt, dt, lay = a[7:16]
    elif entry == "x3d_stem_bwd":          # g, yraw, relu_scale_shift, coef, x, w_s, w_t, dw_s, dw_t, N, Cin, T, H, W, Cout, KT, dtype, x_layout
        ops_, flags = (a[0], a[1], a[4]), nz(a[2], STEM_NAME_RELU_SS)
        n, cin, t, h, w, cout, kt, dt, lay = a[9:18]
    else:
        raise X3DHipError(f"{entry} is not a stem entry point")
    ops_ = tuple(ops_) + (None,) * (4 - len(ops_))
    return (entry.encode(),) + ops_ + (flags, n, cin, t, h, w, cout, kt, dt, lay)


def stem_kernel_name(entry, *args):
    """Instantiation the stem entry point `entry` would launch for its positional arguments `args` (C ABI order, the stream
    excluded; no launch, no GPU needed).  Raises where the entry refuses the launch."""
    buf = C.create_string_buffer(128)
    rc = load().x3d_stem_kernel_name(*stem_launch_query(entry, args), buf, 128)
    if rc != 0:
        raise X3DHipError(load().x3d_last_error().decode())
    return buf.value.decode()


def kernel_name(args):
    """pw_kernel_name / dw3d_kernel_name by struct type."""
    return dw3d_kernel_name(args) if isinstance(args, (Dw3dFwdArgs, Dw3dBwdArgs)) else pw_kernel_name(args)


def dtype_code(dt):
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16
    raise X3DHipError(f"unsupported activation dtype {dt}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr():
    return torch.cuda.current_stream().cuda_stream


def check(status, what=""):
    if status != 0:
        msg = load().x3d_last_error()
        raise X3DHipError(f"{what} failed ({status}): {msg.decode() if msg else ''}")


def call(name, *args):
    """Call a plain-argument entry point on the current stream."""
    lib = load()
    check(getattr(lib, name)(*args, stream_ptr()), name)


def call_struct(name, struct):
    lib = load()
    check(getattr(lib, name)(C.byref(struct), stream_ptr()), name)


def call_struct_dil(name, struct, dilation):
    """x3d_dw3d_fwd_dil / x3d_dw3d_bwd_dil on the current stream: the struct, then the dilation"""
    lib = load()
    check(getattr(lib, name)(C.byref(struct), int(dilation), stream_ptr()), name)


def stats_layout(c: int):
    """(replicas, stride in doubles) of a statistics accumulator for c channels (include/x3d_hip.h)."""
    lib = load()
    return int(lib.x3d_stats_replicas()), int(lib.x3d_stats_stride(int(c)))
