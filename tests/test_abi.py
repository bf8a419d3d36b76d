"""The C-ABI library loads on a CPU-only host and exports exactly what include/x3d_hip.h declares.
(No compute calls here: there is no GPU in the build container.)"""
import os
import re

from x3d_tf_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "x3d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(x3d_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert _declared() == hip.exported_symbols()


def test_library_exports_every_declared_symbol():
    lib = hip.load()
    for name in _declared():
        assert getattr(lib, name) is not None
    header = int(re.search(r"#define X3D_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "x3d_hip.h")).read()).group(1))
    assert lib.x3d_version() == header == hip.ABI_VERSION
    assert lib.x3d_last_error() is not None


def test_product_library_reads_no_environment():
    """the kernel-selection A/B switches exist only in -DX3D_EXPERIMENTS builds (csrc/common.h x3d_env_int): the product
    library must not even import getenv, so no X3D_* variable can change which kernel a launch takes"""
    import shutil
    import subprocess
    import pytest
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    if not os.path.exists(nm):
        pytest.skip("no nm in this image")
    from x3d_tf_amd import build
    if "-DX3D_EXPERIMENTS" in build.FLAGS:
        pytest.skip("experiments build")
    out = subprocess.run([nm, "-D", "--undefined-only", hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in out


def test_stale_library_is_refused(tmp_path, monkeypatch):
    """a library built from another version of the header must not load (its argument lists may have shifted)"""
    import pytest
    monkeypatch.setattr(hip, "ABI_VERSION", hip.ABI_VERSION + 1)
    with pytest.raises(hip.X3DHipError, match="ABI version"):
        hip.load(hip.LIB_PATH)


def _header_structs():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "x3d_hip.h")).read(), flags=re.S)
    return re.findall(r"typedef struct \{[^{}]*\}\s*(x3d_\w+)\s*;", text)


def _hip_structs():
    """C name -> class, from the public names of hip (x3d_pw_fwd_args <- PwFwdArgs)"""
    import ctypes
    return {"x3d_" + re.sub(r"(?<!^)([A-Z])", r"_\1", n).lower(): c for n, c in vars(hip).items()
            if not n.startswith("_") and isinstance(c, type) and issubclass(c, ctypes.Structure)}


def test_every_header_struct_has_a_class():
    assert len(_header_structs()) == 16
    assert sorted(_header_structs()) == sorted(_hip_structs())


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof, and offset and size of every field, of all argument structs: what the C++ compiler makes of include/x3d_hip.h
    (tests/abi_layout_probe.cpp, field lists written out by hand) == what ctypes makes of the classes hip.py derives from it"""
    import ctypes
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import pytest
        pytest.skip("hipcc not available")
    exe = tmp_path / "abi_layout_probe"
    r = subprocess.run([hipcc, "-x", "c++", "-O0", os.path.join(ROOT, "tests", "abi_layout_probe.cpp"),
                        "-I" + os.path.join(ROOT, "include"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    compiled = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        name, *nums = line.split()
        compiled[name] = tuple(int(n) for n in nums)
    ours = {}
    for cname, cls in _hip_structs().items():
        ours[cname] = (ctypes.sizeof(cls),)
        for f, _ in cls._fields_:
            ours[f"{cname}.{f}"] = (getattr(cls, f).offset, getattr(cls, f).size)
    assert sorted(n for n in compiled if "." not in n) == sorted(_header_structs())    # the probe covers every struct
    assert compiled == ours, {k: (compiled.get(k), ours.get(k)) for k in set(compiled) | set(ours) if compiled.get(k) != ours.get(k)}


def test_pinned_signatures():
    """argument and return types of one entry point per mapping rule, and of the long long / double / float positions a
    32-bit or wrong-width slot would corrupt silently, written out literally"""
    from ctypes import POINTER as P, c_char_p, c_double as d, c_float as f, c_int as i, c_longlong as ll, c_size_t, c_uint32, c_void_p as vp
    sigs = {
        "x3d_version": ([], i),
        "x3d_last_error": ([], c_char_p),
        "x3d_stats_stride": ([i], ll),
        "x3d_tail_fwd": ([vp, vp, vp, vp, vp, i, i, ll, i, vp], i),
        "x3d_tail_fwd_bn": ([vp, P(hip.BnFold), vp, P(hip.BnFold), vp, i, i, ll, i, vp], i),
        "x3d_pool_fwd": ([vp, vp, vp, i, i, ll, i, vp], i),
        "x3d_subsample2": ([vp, vp, ll, i, i, i, vp], i),
        "x3d_sgd_nesterov": ([vp, vp, vp, vp, f, f, f, f, ll, vp], i),
        "x3d_adam": ([vp, vp, vp, vp, vp, f, f, f, f, f, f, ll, ll, vp], i),
        "x3d_nthwc_to_ncthw": ([vp, i, vp, i, i, i, ll, vp], i),
        "x3d_bn_finalize": ([vp, d, vp, vp, vp, vp, f, f, i, vp, vp, i, vp], i),
        "x3d_se_fwd": ([vp, d, vp, vp, vp, vp, vp, vp, vp, i, i, i, vp], i),
        "x3d_dense_fwd": ([vp, vp, f, vp, vp, vp, i, i, i, i, vp], i),
        "x3d_mix_clips": ([vp, vp, i, f, i, i, i, i, i, i, i, i, i, i, vp], i),
        "x3d_mix_targets": ([vp, vp, vp, vp, f, f, i, i, vp], i),
        "x3d_pw_fwd": ([P(hip.PwFwdArgs), vp], i),
        "x3d_pw_kernel_name": ([P(hip.PwFwdArgs), P(hip.PwDgradArgs), P(hip.PwWgradArgs), P(hip.PwBwdArgs), c_char_p, i], i),
        "x3d_dw_slab_reduce": ([P(hip.DwReduceJob), i, vp], i),
        "x3d_bn_eval_coef_batched": ([vp, i, f, vp], i),      # items: device memory
        "x3d_pw_pack_weights": ([vp, i, i, vp], i),            # items: device memory
        "x3d_train_resized_hw": ([i, i, f, P(i), P(i)], i),
        "x3d_jpeg_parse": ([vp, vp, i, P(hip.JpegImage), P(ll)], i),
        "x3d_crc32c": ([c_char_p, c_size_t, c_uint32], c_uint32),
    }
    lib = hip.load()
    for name, (argtypes, restype) in sigs.items():
        fn = getattr(lib, name)
        assert (list(fn.argtypes), fn.restype) == (argtypes, restype), name
    # pointer fields of the structs: addresses held as integers, except the BatchNorm fold x3d_dw3d_fwd takes by reference
    fields = {cls: dict(cls._fields_) for cls in (hip.PwDgradArgs, hip.PwWgradArgs, hip.PwBwdArgs, hip.Dw3dFwdArgs,
                                                  hip.JpegDecodeArgs, hip.BnFold, hip.JpegImage)}
    for cls in (hip.PwDgradArgs, hip.PwWgradArgs, hip.PwBwdArgs):
        assert fields[cls]["coef_fold"] is vp
    assert fields[hip.JpegDecodeArgs]["images"] is vp and fields[hip.JpegDecodeArgs]["host_images"] is vp
    assert fields[hip.JpegDecodeArgs]["scratch_bytes"] is ll and fields[hip.JpegImage]["data_off"] is ll
    assert fields[hip.Dw3dFwdArgs]["in_bn"] is P(hip.BnFold)
    assert fields[hip.BnFold]["count"] is d and fields[hip.BnFold]["eps"] is f


def test_header_parser_is_strict():
    """a declaration the parser does not understand is an error that names it, never a silent skip"""
    import pytest
    good = "#define X3D_ABI_VERSION 7\ntypedef struct {\n  const float* w;\n  int N, C;\n} x3d_t;\nint x3d_f(const x3d_t* a, void* stream);\n"
    consts, structs, sigs = hip._parse_header(good)
    assert consts == {"ABI_VERSION": 7} and list(sigs) == ["x3d_f"] and [n for n, _ in structs["x3d_t"]._fields_] == ["w", "N", "C"]
    bad = {
        "int x3d_g(const half* x, int n);": r"line 7.*half.*x3d_g",                     # unknown pointee
        "int x3d_g(unsigned n);": r"line 7.*unsigned.*x3d_g",                           # unknown scalar
        "int x3d_g(int (*cb)(int), int n);": r"line 7.*x3d_g",                          # function pointer
        "int x3d_g(int n)\nint x3d_h(int n);": r"line 7.*x3d_g",                        # missing semicolon
        "typedef struct { float* a, b; } x3d_u;": r"line 7.*float\* a, b",               # pointer declarator list
        "typedef struct {\n  int n;\n  short s;\n} x3d_u;": r"line 9.*short s",              # unknown field type: its own line
        "typedef struct { int n; int m } x3d_u;": r"line 7.*int m",                     # field without a semicolon
        "enum x3d_e { A, B };": r"line 7.*enum",                                        # not a prototype or struct
        "#define X3D_SCALE 1.5f": r"line 7.*X3D_SCALE",                                 # constant that is not an integer
    }
    for decl, message in bad.items():
        with pytest.raises(hip.X3DHipError, match=message):
            hip._parse_header(good + decl + "\nint x3d_tail(int n);\n")


def test_missing_library_fails_loudly(tmp_path):
    import pytest
    with pytest.raises(hip.X3DHipError):
        hip.load(str(tmp_path / "libx3d_hip.so"))


def test_dw3d_kernel_name_dry_run():
    """x3d_dw3d_kernel_name runs the depthwise dispatch without launching (no GPU needed): the names are the
    instantiations bench.py's roofline row and the rocprofv3 summaries refer to."""
    f = hip.Dw3dFwdArgs()
    f.x = f.w = f.y = 256
    f.dtype = hip.BF16
    f.N, f.C, f.T, f.H, f.W, f.stride = 64, 54, 16, 112, 112, 2
    assert hip.dw3d_kernel_name(f) == "dw3d_fwd_di_kernel<bf16, 2>"             # stride 2, strips of four: the de-interleaved LDS plane
    b = hip.Dw3dBwdArgs()
    b.dv = b.braw = b.coef_nc = b.araw = b.a_scale_shift = b.w = b.ga = b.a_sums = b.dw = 256
    b.dtype = hip.BF16
    b.N, b.C, b.T, b.H, b.W, b.stride = 64, 108, 16, 56, 56, 1
    assert hip.dw3d_kernel_name(b) == "dw3d_bwd_s1r_kernel<bf16, 8, 1, 6>"      # dw_s1.hip
    b.C, b.H, b.W, b.stride = 54, 112, 112, 2
    assert hip.dw3d_kernel_name(b) == "dw3d_bwd_s2r_kernel<bf16, 8, 2, 6>"      # dw_s2.hip: the headline's largest launches
    b.dtype = hip.F32
    assert hip.dw3d_kernel_name(b).startswith("dw3d_bwd_kernel<float, 2, 2, "), hip.dw3d_kernel_name(b)   # fp32 storage keeps the older kernels
    f.stride = 3
    import pytest
    with pytest.raises(hip.X3DHipError):
        hip.dw3d_kernel_name(f)
    assert hip.load().x3d_crc32c(b"123456789", 9, 0) == 0xE3069283


def test_cpp_client_links_against_the_c_abi(tmp_path):
    """tools/bench_dw3d.cpp is a C++ client of include/x3d_hip.h with no Python / torch in the loop: it must compile
    and link against libx3d_hip.so (run on a GPU box: profiles/r01e_bench_dw3d_cabi.txt)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        import pytest
        pytest.skip("hipcc not available")
    out = tmp_path / "bench_dw3d"
    libdir = os.path.join(ROOT, "x3d-tf_amd")
    r = subprocess.run([hipcc, "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tools", "bench_dw3d.cpp"),
                        "-I" + os.path.join(ROOT, "include"), "-L" + libdir, "-lx3d_hip", "-o", str(out)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.exists()
