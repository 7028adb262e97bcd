"""spmv_scpa_amd -- Python face of the MI355X SpMV engine.

A thin ctypes binding over ``lib/libspmv_scpa_amd.so`` (host C API + HIP
kernels for gfx950 behind a C ABI; headers in ``include/``).  The names
mirror the reference's C host API (``io_load_csr``, ``csr_to_hll``,
``bench_csr_serial`` ... reference include/csr.h:29-49, hll.h:54-70) so the
tests read like calls into the reference.

There is no Python or CPU fallback for the GPU path: if the shared library
is missing the import fails, and without a GPU every ``*_hip`` call raises
``OSError(ENODEV)``.
"""
import atexit
import collections
import ctypes as C
import os
import re
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "lib", "libspmv_scpa_amd.so")
# harness knob (tools/README.md): the ablations flavour of the library
# (`make -C spmv_scpa_amd/csrc abl`), for tools/sweep.py and the PMC scripts
if os.environ.get("SPMV_LIB"):
    LIB_PATH = os.path.abspath(os.environ["SPMV_LIB"])
INCLUDE_DIR = os.path.join(ROOT, "include")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "%s not found: build it with `python -c 'import __graft_entry__ as g; "
        "g.build()'` (make -C spmv_scpa_amd/csrc). There is no fallback path."
        % LIB_PATH)


def _torch_lib_dir():
    """torch/lib of an installed PyTorch WITHOUT importing it, or None"""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return None
    d = os.path.join(list(spec.submodule_search_locations)[0], "lib")
    return d if os.path.isdir(d) else None


def _bind_the_rocm_runtime():
    """ONE copy of the ROCm runtime per process, no global symbols -- and, by
    default, the runtime the library was BUILT for.  -> ("system" | "torch",
    [bundled libraries preloaded] or None)

    Why one copy (rounds 2-4): this module once loaded libspmv_scpa_amd.so
    with RTLD_GLOBAL; the symbols of its dependency closure (librccl ->
    librocm_smi64) became process-wide, a later `import torch` bound against
    them, objects ended up destroyed by two owners and glibc aborted inside
    exit() (`double free or corruption (!prev)`; no GPU, handle or kernel
    involved -- tests/test_rocm_runtime_once.py reproduces it with imports
    alone).  Hence RTLD_LOCAL.  And PyTorch's ROCm wheels bundle their own
    libamdhip64 / librccl / libhsa-runtime64 under torch/lib and ask for them
    by UNVERSIONED file name (RPATH $ORIGIN), which the loader does not take
    for /opt/rocm's libamdhip64.so.7: torch and this library in one process
    map TWO runtimes unless one of them gives way.

    Which copy (round 6): the library is compiled by
    /opt/rocm's hipcc (HIP 7.2); torch 2.10's wheel bundles HIP 7.0.  Until
    round 5 torch's copy was always preloaded, so every Python-side run --
    tests and bench -- executed 7.2-built code objects on a 7.0 runtime.  Now:
      * torch NOT imported yet (default): nothing is preloaded; the library's
        RUNPATH binds /opt/rocm's runtime, the one it was built against
        (`rocm_runtime_report()`: hip_built == hip_runtime).  A later `import
        torch` in the same process would map the second runtime, so it is
        REFUSED with an ImportError that says what to do (import torch first,
        or SPMV_ROCM_RUNTIME=torch) -- loud, not a crash at exit.
      * torch already imported (bench.py's ranks, the dist workers: they need
        torch.distributed): its runtime is the process's runtime; the
        library's versioned DT_NEEDED names resolve to the mapped copies by
        SONAME.  A major.minor difference to the build is warned about at the
        first device query and flagged (`rocm.mismatch`) in the bench line.
      * SPMV_ROCM_RUNTIME=torch: preload torch's copies now (a process that
        will import torch LATER); =system: never share (the default's
        behaviour, stated).  SPMV_NO_TORCH_PRELOAD=1 (older knob) = system."""
    import sys
    mode = os.environ.get("SPMV_ROCM_RUNTIME", "").strip().lower() or "auto"
    if mode not in ("auto", "system", "torch"):
        raise ImportError("SPMV_ROCM_RUNTIME=%r: auto, system or torch" % mode)
    if os.environ.get("SPMV_NO_TORCH_PRELOAD") and mode == "auto":
        mode = "system"
    if "torch" in sys.modules:
        if mode == "system":
            import warnings
            warnings.warn("spmv_scpa_amd: SPMV_ROCM_RUNTIME=system, but torch "
                          "is already imported: its bundled ROCm runtime is "
                          "this process's runtime", RuntimeWarning)
        return "torch", None
    if mode != "torch":
        return "system", None
    libdir = _torch_lib_dir()
    if not libdir:
        return "system", None
    # A bundled copy can stand in for /opt/rocm's only if the loader will
    # take it for the name this library asks for: its DT_SONAME must equal our
    # DT_NEEDED entry (libamdhip64.so.7, librccl.so.1, libgomp.so.1).  Another
    # SONAME (a torch wheel built for another ROCm major) would map BOTH
    # runtimes -- the very state this function removes -- so such a copy is
    # not preloaded, and the import says so.
    _, needed = _elf_dynamic(LIB_PATH)
    loaded = []
    for name in ("libgomp.so", "libamdhip64.so", "librccl.so"):
        path = os.path.join(libdir, name)
        if not os.path.exists(path):
            continue
        soname, _ = _elf_dynamic(path)
        want = [n for n in needed if n.startswith(name)]
        if want and soname != want[0]:
            import warnings
            warnings.warn(
                "spmv_scpa_amd: torch bundles %s with SONAME %r but "
                "libspmv_scpa_amd.so needs %r: not sharing torch's ROCm "
                "runtime (importing torch later in this process would map a "
                "second one)" % (name, soname, want[0]), RuntimeWarning)
            return ("torch", loaded) if loaded else ("system", None)
        C.CDLL(path, mode=C.RTLD_LOCAL)
        loaded.append(path)
    return ("torch", loaded) if loaded else ("system", None)


class _RefusingLoader:
    def __init__(self, why):
        self.why = why

    def create_module(self, spec):
        raise ImportError(self.why)

    def exec_module(self, module):
        raise ImportError(self.why)


class _NoTorchAfterTheSystemRuntime:
    """meta-path guard installed when the library is bound to /opt/rocm's
    runtime and PyTorch bundles its own: `import torch` now would map a second
    HIP / HSA / RCCL runtime into the process (two owners of one device
    state: measured on an MI355X with this guard lifted, torch's copy then
    answers "No HIP GPUs are available" once this library has the device).
    Refused, loudly, with the two ways out.  Only the IMPORT is
    refused: importlib.util.find_spec("torch") still answers (the real spec,
    with a loader that raises)."""

    def find_spec(self, name, path=None, target=None):
        if name != "torch":
            return None
        import sys
        spec = None
        for f in sys.meta_path:
            if f is self or not hasattr(f, "find_spec"):
                continue
            spec = f.find_spec(name, path, target)
            if spec is not None:
                break
        if spec is None:
            return None
        spec.loader = _RefusingLoader(
            "spmv_scpa_amd is bound to the system ROCm runtime (%s); "
            "PyTorch bundles its own copy and importing it now would map "
            "a second runtime into this process.  Import torch BEFORE "
            "spmv_scpa_amd (the library then shares torch's runtime), or "
            "set SPMV_ROCM_RUNTIME=torch."
            % ((mapped_rocm_runtimes().get("libamdhip64.so") or ["?"])[0]))
        return spec


def allow_torch_import():
    """lift the guard: for a process that only BUILT or inspected the library
    (no device work through it) and goes on to import torch for its own
    purposes -- __graft_entry__.build() calls this.  A process that has used
    the GPU through this library must not: torch's runtime copy would find
    the device taken."""
    import sys
    sys.meta_path[:] = [f for f in sys.meta_path
                        if not isinstance(f, _NoTorchAfterTheSystemRuntime)]


def _guard_against_a_second_runtime():
    import sys
    if ROCM_RUNTIME_BOUND != "system":
        return False
    libdir = _torch_lib_dir()
    if not libdir or not os.path.exists(os.path.join(libdir,
                                                     "libamdhip64.so")):
        return False  # no torch, or a torch that uses the system runtime
    sys.meta_path.insert(0, _NoTorchAfterTheSystemRuntime())
    return True


def _elf_dynamic(path):
    """(DT_SONAME or None, [DT_NEEDED ...]) of an ELF64 little-endian shared
    object, read from its section headers; (None, []) when it is not one"""
    import struct
    try:
        with open(path, "rb") as f:
            eh = f.read(64)
            if eh[:6] != b"\x7fELF\x02\x01":
                return None, []
            shoff, = struct.unpack_from("<Q", eh, 0x28)
            shentsize, shnum = struct.unpack_from("<HH", eh, 0x3A)
            f.seek(shoff)
            sh = [struct.unpack_from("<IIQQQQIIQQ", f.read(shentsize))
                  for _ in range(shnum)]
            dyn = next((s for s in sh if s[1] == 6), None)  # SHT_DYNAMIC
            if dyn is None or dyn[6] >= len(sh):
                return None, []
            f.seek(sh[dyn[6]][4])
            strtab = f.read(sh[dyn[6]][5])
            f.seek(dyn[4])
            raw = f.read(dyn[5])
    except (OSError, struct.error):
        return None, []

    def name(off):
        return strtab[off:strtab.index(b"\0", off)].decode()

    soname, needed = None, []
    for i in range(0, len(raw) - 15, 16):
        tag, val = struct.unpack_from("<qQ", raw, i)
        if tag == 0:
            break
        if tag == 1:
            needed.append(name(val))
        elif tag == 14:
            soname = name(val)
    return soname, needed


def mapped_rocm_runtimes():
    """{library: sorted real paths} of the HIP / RCCL / HSA runtimes mapped
    into this process right now (/proc/self/maps): one path each in a healthy
    process, whatever the import order"""
    seen = {}
    try:
        with open("/proc/self/maps") as f:
            lines = f.read().splitlines()
    except OSError:
        lines = []
    for line in lines:
        m = re.search(r"(/\S+\.so\S*)$", line.strip())
        if m:
            base = re.sub(r"\.so.*", ".so", os.path.basename(m.group(1)))
            if base in ("libamdhip64.so", "librccl.so", "libhsa-runtime64.so"):
                seen.setdefault(base, set()).add(os.path.realpath(m.group(1)))
    return {k: sorted(v) for k, v in seen.items()}


def _fmt_hip(v):
    return "%d.%d.%d" % (v // 10_000_000, v // 100_000 % 100, v % 100_000)


def rocm_runtime_report():
    """what this process runs the library on: the HIP version it was built
    against, the one the bound runtime reports, which copy that is (the
    system's or torch's bundled one), every runtime copy mapped, and
    `mismatch`: built and bound differ in major.minor (bench.py prints it)"""
    built = _lib.spmv_hip_build_version()
    run = _lib.spmv_hip_runtime_version()
    maps = mapped_rocm_runtimes()
    lib = (maps.get("libamdhip64.so") or [None])[0]
    return {"hip_built": _fmt_hip(built),
            "hip_runtime": _fmt_hip(run) if run > 0 else None,
            "bound": ROCM_RUNTIME_BOUND,
            "shared_with_torch": ROCM_RUNTIME_BOUND == "torch",
            "mismatch": bool(run > 0 and run // 100_000 != built // 100_000),
            # copies of the HIP / RCCL / HSA runtime mapped: 1 each when healthy
            "runtimes_mapped": max([len(v) for v in maps.values()] or [0]),
            "hip_from": "torch/lib" if lib and "/torch/lib/" in lib else lib}


def _check_the_bound_runtime():
    """after loading: exactly one copy of each runtime library mapped (a file
    read; no HIP call is made at import -- a process that only imports, like
    a launcher, must not initialise the GPU runtime)"""
    import warnings
    twice = {k: v for k, v in mapped_rocm_runtimes().items() if len(v) > 1}
    if twice:
        warnings.warn("spmv_scpa_amd: more than one copy of the ROCm runtime "
                      "is mapped into this process: %r -- objects may be "
                      "destroyed by two owners at exit" % (twice,),
                      RuntimeWarning)
    return not twice


_versions_checked = False


def _check_the_hip_version_once():
    """first device query: the HIP runtime the library is bound to should be
    the one it was built with -- a different major.minor (torch's bundled
    runtime in a process that needs torch) is warned about, loudly, once, and
    flagged by rocm_runtime_report()["mismatch"]"""
    global _versions_checked
    if _versions_checked:
        return
    _versions_checked = True
    built = _lib.spmv_hip_build_version()
    run = _lib.spmv_hip_runtime_version()
    if run > 0 and run // 100_000 != built // 100_000:
        import warnings
        warnings.warn("spmv_scpa_amd: built against HIP %s, bound to a HIP %s "
                      "runtime (%s): gfx950 code objects of one toolchain on "
                      "another runtime -- works today, nothing guarantees it"
                      % (_fmt_hip(built), _fmt_hip(run),
                         "torch's bundled copy: this process imported torch"
                         if ROCM_RUNTIME_BOUND == "torch" else
                         "the system's"), RuntimeWarning)


ROCM_RUNTIME_BOUND, ROCM_RUNTIME_SHARED_WITH_TORCH = _bind_the_rocm_runtime()
_lib = C.CDLL(LIB_PATH, mode=C.RTLD_LOCAL)  # never RTLD_GLOBAL: see above
ROCM_TORCH_IMPORT_GUARDED = _guard_against_a_second_runtime()
for _n in ("spmv_hip_build_version", "spmv_hip_runtime_version"):
    getattr(_lib, _n).restype = C.c_int
    getattr(_lib, _n).argtypes = []
ROCM_RUNTIME_ONCE = _check_the_bound_runtime()

MAX_NAME = 64
HACK_SIZE = 32
SYNTH_BANDED, SYNTH_RANDOM, SYNTH_RAGGED, SYNTH_KKT, SYNTH_STENCIL = 0, 1, 2, 3, 4
SYNTH_POWERLAW, SYNTH_HUB = 5, 6  # webbase/amazon/roadNet class, dc1 class
NUM_CSR_KERNELS = 5
NUM_HLL_KERNELS = 4
NUM_CSR_KERNELS_ALL = 6  # + the 2-D blocked path (SPMV_CSR_KERNEL_PANELS)
NUM_HLL_KERNELS_ALL = 5
#: extra kernel ids: the column-panel path (spmv_engine.h)
CSR_KERNEL_PANELS = 5
HLL_KERNEL_PANELS = 4
CSR_KERNEL_NAMES = ["thread_row", "wave_row", "subwave_row", "block_row",
                    "stream"]
HLL_KERNEL_NAMES = ["threads_row_major", "threads_col_major", "wave_block",
                    "subwave_row"]
#: names including the extra 2-D blocked path
CSR_KERNEL_LABELS = CSR_KERNEL_NAMES + ["tile_panels"]
HLL_KERNEL_LABELS = HLL_KERNEL_NAMES + ["tile_panels"]
#: layout each HLL kernel expects (reference main.c:324-325)
HLL_KERNEL_COL_MAJOR = [False, True, True, False]

_ip = C.POINTER(C.c_int)
_dp = C.POINTER(C.c_double)


# ---------------------------------------------------------------- structs
class SparseCSR(C.Structure):
    _fields_ = [("name", C.c_char * MAX_NAME), ("M", C.c_int), ("N", C.c_int),
                ("NZ", C.c_int), ("IRP", _ip), ("JA", _ip), ("AS", _dp)]


class EllpackBlock(C.Structure):
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("NZ", C.c_int),
                ("max_NZ", C.c_int), ("JA", _ip), ("AS", _dp)]


class SparseHLL(C.Structure):
    _fields_ = [("name", C.c_char * MAX_NAME), ("M", C.c_int), ("N", C.c_int),
                ("NZ", C.c_int), ("hack_size", C.c_int),
                ("num_blocks", C.c_int), ("blocks", C.POINTER(EllpackBlock))]


class Vec(C.Structure):
    _fields_ = [("len", C.c_size_t), ("data", _dp)]


class Bench(C.Structure):
    _fields_ = [("duration_ms", C.c_double), ("gflops", C.c_double),
                ("data", Vec)]


class BenchOmp(C.Structure):
    _fields_ = [("bench", Bench), ("name", C.c_char * MAX_NAME),
                ("num_threads", C.c_int)]


class BenchHip(C.Structure):
    _fields_ = [("bench", Bench), ("waves_per_block", C.c_int)]


class LaunchOpts(C.Structure):
    _fields_ = [("waves_per_block", C.c_int), ("group", C.c_int),
                ("variant", C.c_int), ("reserved", C.c_int * 5)]


class PanelOpts(C.Structure):
    """spmv_panel_opts (include/spmv_engine.h)"""
    _fields_ = [("struct_size", C.c_int),
                ("sched", C.c_int), ("panel_cols", C.c_int),
                ("tile_rows", C.c_int), ("sweep_wgs_per_cu", C.c_int),
                ("reserve_cus", C.c_int), ("lds_min", C.c_int),
                ("tile_order", C.c_int), ("sweep_layout", C.c_int),
                ("bucket_order", C.c_int), ("deterministic", C.c_int)]


class CgInfo(C.Structure):
    """spmv_cg_info (include/spmv_engine.h): one column of a cg() solve"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int),
                ("rr", C.c_double), ("bb", C.c_double)]


class CglsInfo(C.Structure):
    """spmv_cgls_info (include/spmv_engine.h): one column of a cgls() solve"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int),
                ("ss", C.c_double), ("atb", C.c_double), ("rr", C.c_double)]


class MinresInfo(C.Structure):
    """spmv_minres_info (include/spmv_engine.h): one column of a minres()
    solve"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int),
                ("pp", C.c_double), ("bn2", C.c_double), ("rr", C.c_double),
                ("bb", C.c_double)]


class GmresInfo(C.Structure):
    """spmv_gmres_info (include/spmv_engine.h): one column of a gmres()
    solve"""
    _fields_ = [("status", C.c_int), ("iterations", C.c_int),
                ("restarts", C.c_int), ("reserved", C.c_int),
                ("rr", C.c_double), ("est", C.c_double), ("bb", C.c_double)]


class Ic0Info(C.Structure):
    """spmv_ic0_info (include/spmv_engine.h): one CsrDevice.ic0()"""
    _fields_ = [("levels", C.c_int), ("launches", C.c_int),
                ("entries", C.c_int64), ("bad_pivots", C.c_int64)]


class Ilu0Info(C.Structure):
    """spmv_ilu0_info (include/spmv_engine.h): one CsrDevice.ilu0()"""
    _fields_ = [("levels", C.c_int), ("launches", C.c_int),
                ("entries", C.c_int64), ("bad_pivots", C.c_int64)]


class ColourInfo(C.Structure):
    """spmv_colour_info (include/spmv_engine.h): one CsrDevice.colour()"""
    _fields_ = [("colours", C.c_int), ("rounds", C.c_int),
                ("widest", C.c_int), ("narrowest", C.c_int)]


class AggregateInfo(C.Structure):
    """spmv_aggregate_info (include/spmv_engine.h): one CsrDevice.aggregate()"""
    _fields_ = [("aggregates", C.c_int), ("roots", C.c_int),
                ("rounds", C.c_int), ("widest", C.c_int),
                ("singletons", C.c_int)]


AMG_MAX_LEVELS = 32


class AmgSummary(C.Structure):
    """spmv_amg_summary (include/spmv_engine.h): AmgHierarchy.info"""
    _fields_ = [("levels", C.c_int), ("sweeps", C.c_int),
                ("coarse_sweeps", C.c_int), ("kmax", C.c_int),
                ("rows", C.c_int * AMG_MAX_LEVELS),
                ("rounds", C.c_int * AMG_MAX_LEVELS),
                ("aggregates", C.c_int * AMG_MAX_LEVELS),
                ("launches", C.c_int),
                ("entries", C.c_int64 * AMG_MAX_LEVELS),
                ("rho", C.c_double * AMG_MAX_LEVELS),
                ("omega", C.c_double * AMG_MAX_LEVELS),
                ("complexity", C.c_double), ("scratch_bytes", C.c_int64)]


class SpgemmInfo(C.Structure):
    """spmv_spgemm_info (include/spmv_engine.h): one CsrDevice.matmul()"""
    _fields_ = [("products", C.c_int64), ("widest", C.c_int64),
                ("rows_in_bin", C.c_int64 * 4), ("nz", C.c_int)]


class AddInfo(C.Structure):
    """spmv_add_info (include/spmv_engine.h): one CsrDevice.add()"""
    _fields_ = [("nz", C.c_int), ("matched", C.c_int64),
                ("widest", C.c_int64), ("rows_in_bin", C.c_int64 * 2)]


_CSRp = C.POINTER(SparseCSR)
_HLLp = C.POINTER(SparseHLL)


def _sig(name, restype, *argtypes):
    fn = getattr(_lib, name)
    fn.restype = restype
    fn.argtypes = list(argtypes)
    return fn


# ---------------------------------------------------------------- errors
def _is_err(addr):
    """IS_ERR of include/err.h on an integer address."""
    return addr is not None and addr >= (1 << 64) - 4095


def _check(rc, what):
    if rc < 0:
        raise OSError(-rc, "%s: %s" % (what, os.strerror(-rc)))
    return rc


def _ptr_or_raise(p, what):
    addr = C.cast(p, C.c_void_p).value
    if addr is None:
        raise OSError(0, "%s returned NULL" % what)
    if _is_err(addr):
        code = addr - (1 << 64)
        raise OSError(-code, "%s: %s" % (what, os.strerror(-code)))
    return p


# ---------------------------------------------------------------- host API
_sig("io_load_csr", _CSRp, C.c_char_p)
_sig("csr_free", None, _CSRp)
_sig("csr_save_bin", C.c_int, _CSRp, C.c_char_p)
_sig("csr_load_bin", _CSRp, C.c_char_p)
_sig("io_load_csr_cached", _CSRp, C.c_char_p)
_sig("csr_alloc", _CSRp, C.c_char_p, C.c_int, C.c_int, C.c_int)
_sig("csr_generate", _CSRp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64,
     C.c_int64, C.c_uint64)
_sig("csr_row_slice", _CSRp, _CSRp, C.c_int, C.c_int)
_sig("extract_matrix_name", None, C.c_char_p, C.c_char_p)
_sig("partition_rows_nnz", _ip, _CSRp, _ip)
_sig("partition_rows_even", _ip, C.c_int, C.c_int, C.c_int)
_sig("partition_rows_nnz_aligned", _ip, _ip, C.c_int, C.c_int, C.c_int)
_sig("partition_synth_rows_nnz", _ip, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_int64, C.c_uint64, C.c_int, C.c_int)
_sig("csr_to_hll", _HLLp, _CSRp, C.c_bool)
_sig("hll_free", None, _HLLp)
_sig("hll_num_slots", C.c_int64, _HLLp)
_sig("hll_is_contiguous", C.c_int, _HLLp)
_sig("vec_put", None, C.POINTER(Vec))
_sig("aligned_malloc", C.c_void_p, C.c_size_t)
_sig("validation_vec_result", C.c_int, Vec, Vec)
_sig("max_rel_err", C.c_double, Vec, Vec, _dp)
for _n in ("bench_csr_serial",):
    _sig(_n, C.c_int, _CSRp, _dp, C.POINTER(Bench))
for _n in ("bench_csr_omp_guided", "bench_csr_omp_nnz_balancing"):
    _sig(_n, C.c_int, _CSRp, _dp, C.POINTER(BenchOmp))
for _n in ("bench_hll_serial", "bench_hll_serial_col_major"):
    _sig(_n, C.c_int, _HLLp, _dp, C.POINTER(Bench))
_sig("bench_hll_omp", C.c_int, _HLLp, _dp, C.POINTER(BenchOmp))
for _n in CSR_KERNEL_NAMES:
    _sig("bench_csr_hip_" + _n, C.c_int, _CSRp, _dp, C.POINTER(BenchHip))
    _sig("csr_spmv_hip_" + _n, C.c_double, _CSRp, _dp, _dp, C.c_void_p)
for _n in HLL_KERNEL_NAMES:
    _sig("bench_hll_hip_" + _n, C.c_int, _HLLp, _dp, C.POINTER(BenchHip))
    _sig("hll_spmv_hip_" + _n, C.c_double, _HLLp, _dp, _dp, C.c_void_p)
_sig("spmv_device_sync", C.c_int)
_sig("spmv_event_create", C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_event_record", C.c_int, C.c_void_p, C.c_void_p)
_sig("spmv_event_elapsed_ms", C.c_int, C.c_void_p, C.c_void_p,
     C.POINTER(C.c_float))
_sig("spmv_event_destroy", C.c_int, C.c_void_p)
_sig("spmv_stream_create", C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_stream_destroy", C.c_int, C.c_void_p)
_sig("spmv_graph_begin_capture", C.c_int, C.c_void_p)
_sig("spmv_graph_end_capture", C.c_int, C.c_void_p, C.POINTER(C.c_void_p))
_sig("spmv_graph_end_capture_shape", C.c_int, C.c_void_p,
     C.POINTER(C.c_void_p), _ip, _ip, _ip, _ip)
_sig("spmv_graph_launch", C.c_int, C.c_void_p, C.c_void_p)
_sig("spmv_graph_destroy", C.c_int, C.c_void_p)
_sig("spmv_seam_cache", None, C.c_int)
_sig("spmv_seam_cache_stats", C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long))
_sig("spmv_seam_cache_invalidate", C.c_int, C.c_void_p)
_sig("set_csr_waves_per_block", None, C.c_int)
_sig("set_hll_waves_per_block", None, C.c_int)
_sig("logger_init", C.c_int, C.c_char_p)
_sig("logger_close", None)
_sig("log_csr_serial_benchmark", None, _CSRp, Bench)
_sig("log_hll_serial_benchmark", None, _HLLp, Bench)
_sig("log_csr_omp_benchmark", None, _CSRp, BenchOmp)
_sig("log_hll_omp_benchmark", None, _HLLp, BenchOmp)
_sig("log_csr_hip_benchmark", None, _CSRp, BenchHip, C.c_int)
_sig("log_hll_hip_benchmark", None, _HLLp, BenchHip, C.c_int)
_sig("log_roofline", None, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int,
     C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_double)

# ---------------------------------------------------------------- engine API
_sig("spmv_version", C.c_char_p)
_sig("spmv_build_flavour", C.c_char_p)
_sig("spmv_live_handles", C.c_int)
_sig("spmv_ignored_releases", C.c_long)
_sig("spmv_set_debug", None, C.c_int)
_sig("spmv_handle_generation", C.c_uint64, C.c_void_p)
_sig("spmv_panel_opts_default", None, C.POINTER(PanelOpts))
_sig("spmv_device_count", C.c_int)
_sig("spmv_set_device", C.c_int, C.c_int)
_sig("spmv_get_device", C.c_int)
_sig("spmv_device_info", C.c_int, C.c_int, C.c_char_p, C.c_size_t, _ip,
     C.POINTER(C.c_size_t))
_sig("spmv_dev_mem_info", C.c_int, C.POINTER(C.c_size_t),
     C.POINTER(C.c_size_t))
_sig("spmv_dev_malloc", C.c_int, C.POINTER(C.c_void_p), C.c_size_t)
_sig("spmv_dev_free", C.c_int, C.c_void_p)
_sig("spmv_dev_memset", C.c_int, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p)
_sig("spmv_copy_h2d", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("spmv_copy_d2h", C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)
_sig("spmv_stream_sync", C.c_int, C.c_void_p)
_sig("spmv_dev_fill_synth", C.c_int, C.c_void_p, C.c_int64, C.c_uint64,
     C.c_int64, C.c_void_p)
_sig("spmv_csr_upload", C.c_int, _CSRp, C.POINTER(C.c_void_p))
_sig("spmv_csr_upload_f32", C.c_int, _CSRp, C.POINTER(C.c_void_p))
_sig("spmv_csr_to_f32", C.c_int, C.c_void_p, C.POINTER(C.c_void_p))
_sig("spmv_csr_transpose", C.c_int, C.c_void_p, C.POINTER(C.c_void_p))
_sig("spmv_transpose_plan", C.c_int, C.c_int, C.c_int64, _ip, _ip, _ip,
     C.POINTER(C.c_int64), C.POINTER(C.c_int64))
_sig("spmv_csr_symmetry", C.c_int, C.c_void_p, _ip)
_i64p = C.POINTER(C.c_int64)
_sig("spmv_csr_spgemm", C.c_int, C.c_void_p, C.c_void_p,
     C.POINTER(C.c_void_p), C.POINTER(SpgemmInfo))
_sig("spmv_spgemm_shape", C.c_int, _i64p, _ip, _ip, _ip, _ip, _i64p)
_sig("spmv_spgemm_last_phases", None, _dp)
_sig("spmv_csr_galerkin", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
     C.POINTER(C.c_void_p), C.POINTER(SpgemmInfo))
_sig("spmv_csr_add", C.c_int, C.c_double, C.c_void_p, C.c_double, C.c_void_p,
     C.POINTER(C.c_void_p), C.POINTER(AddInfo))
_sig("spmv_add_shape", C.c_int, _i64p, _ip, _ip, _ip)
_sig("spmv_add_set_class", C.c_int, C.c_int)
_sig("spmv_add_last_phases", None, _dp)
_sig("spmv_csr_from_diag", C.c_int, C.c_int, C.c_void_p,
     C.POINTER(C.c_void_p))
_sig("spmv_csr_scale", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
     C.POINTER(C.c_void_p))
_sig("spmv_csr_trsv_analyse", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
     C.POINTER(C.c_void_p))
_sig("spmv_csr_trsv_analyse_sweeps", C.c_int, C.c_void_p, C.c_int, C.c_int,
     C.c_int, C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_trsv_sweeps", C.c_int, C.c_void_p, _ip, _ip)
_sig("spmv_trsv_info", C.c_int, C.c_void_p, _ip, _ip, _i64p, _ip, _i64p, _ip,
     _i64p)
_sig("spmv_trsv_download", C.c_int, C.c_void_p, _ip, _ip, _ip, _ip, _ip, _dp,
     _dp)
_sig("spmv_trsv_shape", None, _ip, _ip, _ip)
_sig("spmv_trsv_release", None, C.c_void_p)
_sig("spmv_trsv_release_checked", None, C.c_void_p, C.c_uint64)
_sig("spmv_trsv_solve", C.c_int, C.c_void_p, C.POINTER(LaunchOpts), C.c_int,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)
_sig("spmv_csr_ic0", C.c_int, C.c_void_p, C.c_double, C.c_int,
     C.POINTER(C.c_void_p), C.POINTER(Ic0Info))
_sig("spmv_csr_ilu0", C.c_int, C.c_void_p, C.c_double, C.c_int,
     C.POINTER(C.c_void_p), C.POINTER(Ilu0Info))
_sig("spmv_csr_colour", C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p,
     C.c_void_p, C.POINTER(ColourInfo))
_sig("spmv_csr_permute", C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
     C.POINTER(C.c_void_p))
_sig("spmv_csr_aggregate", C.c_int, C.c_void_p, C.c_double, C.c_uint32,
     C.c_int, C.c_void_p, C.POINTER(AggregateInfo))
_sig("spmv_csr_amg_setup", C.c_int, C.c_void_p, C.c_double, C.c_int, C.c_int,
     C.c_int, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_amg_info", C.c_int, C.c_void_p, C.POINTER(AmgSummary))
_sig("spmv_amg_level", C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p),
     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p))
_sig("spmv_amg_last_phases", None, _dp)
_sig("spmv_amg_set_fused", C.c_int, C.c_int)
_sig("spmv_amg_release", None, C.c_void_p)
_sig("spmv_amg_release_checked", None, C.c_void_p, C.c_uint64)
_sig("spmv_amg_apply", C.c_int, C.c_void_p, C.POINTER(LaunchOpts), C.c_int,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p)
_sig("spmv_permute_vectors", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p)
_sig("spmv_csr_generate", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
     C.c_int64, C.c_int64, C.c_uint64, C.POINTER(C.c_void_p))
_sig("spmv_csr_launch_rows", C.c_int, C.c_void_p, C.c_int,
     C.POINTER(LaunchOpts), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
     C.c_void_p)
_sig("spmv_set_panel_schedule", C.c_int, C.c_int)
_sig("spmv_csr_shape", C.c_int, C.c_void_p, _ip, _ip, C.POINTER(C.c_int64))
_sig("spmv_csr_download", C.c_int, C.c_void_p, C.POINTER(_CSRp))
_sig("spmv_hll_upload", C.c_int, _HLLp, C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_hll_upload_f32", C.c_int, _HLLp, C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_hll_from_csr", C.c_int, C.c_void_p, C.c_int,
     C.POINTER(C.c_void_p))
_sig("spmv_hll_launch_blocks", C.c_int, C.c_void_p, C.c_int,
     C.POINTER(LaunchOpts), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
     C.c_void_p)
_sig("spmv_hll_shape", C.c_int, C.c_void_p, _ip, _ip, C.POINTER(C.c_int64),
     _ip, C.POINTER(C.c_int64), _ip)
_sig("spmv_hll_kernel_bytes", C.c_int64, C.c_void_p, C.c_int)
_sig("spmv_cg_work_bytes", C.c_int64, C.c_int, C.c_int)
_sig("spmv_cg_dot_shape", None, _ip, _ip)
_sig("spmv_pcg_work_bytes", C.c_int64, C.c_int, C.c_int)
_sig("spmv_pcg_trsv_work_bytes", C.c_int64, C.c_int, C.c_int)
_sig("spmv_bicgstab_work_bytes", C.c_int64, C.c_int, C.c_int)
_sig("spmv_bicgstab_trsv_work_bytes", C.c_int64, C.c_int, C.c_int)
_sig("spmv_cgls_work_bytes", C.c_int64, C.c_int, C.c_int, C.c_int)
_sig("spmv_minres_work_bytes", C.c_int64, C.c_int, C.c_int)
_sig("spmv_gmres_work_bytes", C.c_int64, C.c_int, C.c_int, C.c_int)
_sig("spmv_debug_sqrt", C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
     C.c_void_p)
# spmv_csr_<name> and spmv_hll_<name>: the same argument types
_TWINS = (
    ("release_checked", None, C.c_void_p, C.c_uint64),
    ("tune_times", C.c_int, C.c_void_p, _dp, C.c_int),
    ("tune_log", C.c_int, C.c_void_p, C.c_char_p, C.c_size_t),
    ("launch", C.c_int,
     C.c_void_p, C.c_int, C.POINTER(LaunchOpts), C.c_void_p, C.c_void_p,
     C.c_void_p),
    ("panels_info", C.c_int, C.c_void_p, _ip, _ip, _ip, C.POINTER(C.c_int64)),
    ("autotune", C.c_int,
     C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _ip, _dp),
    ("panels_layout", C.c_int,
     C.c_void_p, C.POINTER(PanelOpts), C.POINTER(C.c_int)),
    ("panels_set_waves", C.c_int, C.c_void_p, C.c_int),
    ("panels_fit_steps", C.c_int,
     C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)),
    ("panels_set_fit_steps", C.c_int, C.c_void_p, C.c_int64, C.c_int64),
    ("panels_plan", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), _ip, _ip, _ip),
    ("build_panels_opts", C.c_int, C.c_void_p, C.POINTER(PanelOpts)),
    ("build_panels", C.c_int, C.c_void_p, C.c_int),
    ("panels_describe", C.c_int, C.c_void_p, C.c_char_p, C.c_size_t),
    ("panels_tile_rows", C.c_int, C.c_void_p),
    ("build_panels_as", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int),
    ("release_source", C.c_int, C.c_void_p),
    ("panels_schedule", C.c_int, C.c_void_p),
    ("build_panels_like", C.c_int, C.c_void_p, C.c_void_p),
    ("algorithmic_bytes", C.c_int64, C.c_void_p),
    ("value_bytes", C.c_int, C.c_void_p),
    ("release", None, C.c_void_p),
    ("launch_multi", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p),
    ("multi_bytes", C.c_int64, C.c_void_p, C.c_int),
    ("launch_axpby", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_double, C.c_double,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p),
    ("axpby_bytes", C.c_int64, C.c_void_p, C.c_int, C.c_int),
    ("cg", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_double, C.c_int, C.c_int, C.c_void_p,
     C.c_size_t, C.POINTER(CgInfo), C.c_void_p),
    ("pcg", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_int, C.c_int,
     C.c_void_p, C.c_size_t, C.POINTER(CgInfo), C.c_void_p),
    ("pcg_trsv", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
     C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(CgInfo), C.c_void_p),
    ("pcg_amg", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_int, C.c_int,
     C.c_void_p, C.c_size_t, C.POINTER(CgInfo), C.c_void_p),
    ("bicgstab", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_int, C.c_int,
     C.c_void_p, C.c_size_t, C.POINTER(CgInfo), C.c_void_p),
    ("bicgstab_trsv", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double,
     C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(CgInfo), C.c_void_p),
    ("cgls", C.c_int,
     C.c_void_p, C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p,
     C.c_int64, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.c_int,
     C.c_int, C.c_void_p, C.c_size_t, C.POINTER(CglsInfo), C.c_void_p),
    ("minres", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_int, C.c_int,
     C.c_void_p, C.c_size_t, C.POINTER(MinresInfo), C.c_void_p),
    ("gmres", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int,
     C.c_void_p, C.c_size_t, C.POINTER(GmresInfo), C.c_void_p),
    ("gmres_trsv", C.c_int,
     C.c_void_p, C.POINTER(LaunchOpts), C.c_int, C.c_void_p, C.c_int64,
     C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
     C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
     C.POINTER(GmresInfo), C.c_void_p),
    ("diag", C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p),
    ("time", C.c_int,
     C.c_void_p, C.c_int, C.POINTER(LaunchOpts), C.c_void_p, C.c_void_p,
     C.c_int, C.c_int, C.c_size_t, _dp, C.c_void_p),
)
#: spmv_hll_<name> only: compact handles (16-bit column offsets)
_HLL_ONLY = (
    ("to_index16", C.c_int, C.c_void_p, C.POINTER(C.c_void_p)),
    ("index_bytes", C.c_int, C.c_void_p),
    ("download_index16", C.c_int, C.c_void_p, _ip, C.POINTER(C.c_uint16)),
)
for _f, _list in (("csr", _TWINS), ("hll", _TWINS + _HLL_ONLY)):
    for _n, _res, *_args in _list:
        _sig("spmv_%s_%s" % (_f, _n), _res, *_args)

def declared_symbols():
    """Every function name declared in include/*.h (non-inline)."""
    names = set()
    pat = re.compile(r"^[A-Za-z_][\w\s\*]*?\b(\w+)\s*\([^;{]*\)\s*;", re.M | re.S)
    for fn in sorted(os.listdir(INCLUDE_DIR)):
        if not fn.endswith(".h"):
            continue
        text = open(os.path.join(INCLUDE_DIR, fn)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
        for m in pat.finditer(text):
            head = m.group(0)
            if "static" in head.split("(")[0] or "typedef" in head.split("(")[0]:
                continue
            names.add(m.group(1))
    return sorted(names)


def check_symbols():
    """Raise if the library lacks a symbol the headers declare."""
    missing = [n for n in declared_symbols() if not hasattr(_lib, n)]
    if missing:
        raise ImportError("libspmv_scpa_amd.so lacks: %s" % ", ".join(missing))
    return True


# ---------------------------------------------------------------- helpers
def _as_d(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(_dp)


def _take_vec(v):
    """Copy a C vec into numpy and release it (vec_put)."""
    n = v.len
    out = np.ctypeslib.as_array(v.data, (n,)).copy() if n else np.zeros(0)
    _lib.vec_put(C.byref(v))
    return out


def _opts(waves_per_block=0, group=0, variant=0):
    o = LaunchOpts()
    o.waves_per_block = int(waves_per_block)
    o.group = int(group)
    o.variant = int(variant)
    return o


def _cg_dot_shape():
    nwg, t = C.c_int(), C.c_int()
    _lib.spmv_cg_dot_shape(C.byref(nwg), C.byref(t))
    return nwg.value, t.value


#: (workgroups, threads) of the solver's dot product: element i of a vector
#: belongs to slot i mod (workgroups * threads) -- the order of a dot is a
#: function of M and of these two constants (spmv_engine.h, spmv_*_cg)
CG_DOT_SHAPE = _cg_dot_shape()
#: spmv_cg_info.status
CG_CONVERGED, CG_MAXIT, CG_BREAKDOWN = 0, 1, 2
#: one column of a cg() solve
CgResult = collections.namedtuple("CgResult", "status iterations rr bb")


def cg_work_bytes(M, k):
    """bytes of device memory one cg() solve of k systems with M rows needs
    (what `work` must hold at least)"""
    return _check(_lib.spmv_cg_work_bytes(int(M), int(k)),
                  "spmv_cg_work_bytes")


def pcg_work_bytes(M, k):
    """bytes of device memory one pcg() solve of k systems with M rows needs:
    cg_work_bytes and one more set of partial sums"""
    return _check(_lib.spmv_pcg_work_bytes(int(M), int(k)),
                  "spmv_pcg_work_bytes")


def pcg_trsv_work_bytes(M, k):
    """bytes of device memory one pcg_trsv() solve of k systems with M rows
    needs: pcg_work_bytes and one more vector (Z) of 8 k M bytes"""
    return _check(_lib.spmv_pcg_trsv_work_bytes(int(M), int(k)),
                  "spmv_pcg_trsv_work_bytes")


def bicgstab_work_bytes(M, k):
    """bytes of device memory one bicgstab() solve of k systems with M rows
    needs: a base that depends on neither, and six vectors of 8 k M bytes"""
    return _check(_lib.spmv_bicgstab_work_bytes(int(M), int(k)),
                  "spmv_bicgstab_work_bytes")


def bicgstab_trsv_work_bytes(M, k):
    """bytes of device memory one bicgstab_trsv() solve of k systems with M
    rows needs: the base of bicgstab_work_bytes and seven vectors of 8 k M
    bytes (z(P) and z(S) are stored, each in a vector of its own)"""
    return _check(_lib.spmv_bicgstab_trsv_work_bytes(int(M), int(k)),
                  "spmv_bicgstab_trsv_work_bytes")


#: one column of a cgls() solve
CglsResult = collections.namedtuple("CglsResult",
                                    "status iterations ss atb rr")


def cgls_work_bytes(M, N, k):
    """bytes of device memory one cgls() solve of k problems with an M x N
    matrix needs: a base that depends on none of them, and 8 k (2 M + 2 N)
    for R, Q (M rows) and S, P (N rows)"""
    return _check(_lib.spmv_cgls_work_bytes(int(M), int(N), int(k)),
                  "spmv_cgls_work_bytes")


#: one column of a minres() solve
MinresResult = collections.namedtuple("MinresResult",
                                      "status iterations pp bn2 rr bb")


def minres_work_bytes(M, k):
    """bytes of device memory one minres() solve of k systems with M rows
    needs: a base that depends on neither, and six vectors of 8 k M bytes"""
    return _check(_lib.spmv_minres_work_bytes(int(M), int(k)),
                  "spmv_minres_work_bytes")


#: one column of a gmres() solve
GmresResult = collections.namedtuple("GmresResult",
                                     "status iterations restarts rr est bb")
#: the longest cycle of gmres() (GM_MAXM)
GMRES_MAX_RESTART = 64


def gmres_work_bytes(M, k, restart):
    """bytes of device memory one gmres() or gmres_trsv() solve of k systems
    with M rows and cycles of `restart` steps needs: a base that depends on
    restart alone, and restart + 3 vectors of 8 k M bytes (the basis, W, Z)"""
    return _check(_lib.spmv_gmres_work_bytes(int(M), int(k), int(restart)),
                  "spmv_gmres_work_bytes")


#: CsrDevice.symmetry()
SYM_NONE, SYM_PATTERN, SYM_VALUES = 0, 1, 2


def transpose_plan(N, NZ):
    """the geometry CsrDevice.transpose() uses for a source of N columns and
    NZ entries (host arithmetic, no device): dict(passes, digit_bits, tile,
    workgroups, scratch_bytes)"""
    p, d, t = C.c_int(), C.c_int(), C.c_int()
    w, s = C.c_int64(), C.c_int64()
    _check(_lib.spmv_transpose_plan(int(N), int(NZ), C.byref(p), C.byref(d),
                                    C.byref(t), C.byref(w), C.byref(s)),
           "spmv_transpose_plan")
    return dict(passes=p.value, digit_bits=d.value, tile=t.value,
                workgroups=w.value, scratch_bytes=s.value)


#: CsrDevice.spgemm_info of a matmul() / galerkin() result
SpgemmResult = collections.namedtuple("SpgemmResult",
                                      "products widest rows_in_bin nz")


def spgemm_shape():
    """the constants of CsrDevice.matmul() (host, no device): dict(edges,
    tables, teams, lds_bytes, fallback_batch, fallback_bytes) -- a row with ub
    products goes to the first class c = 0..2 with ub <= edges[c], whose
    teams[c] lanes keep its columns in an LDS table of tables[c] slots
    (lds_bytes[c] per workgroup), and to the fallback (class 3) beyond; the
    fallback runs at most fallback_batch rows a launch within fallback_bytes
    of scratch (or one row's)"""
    e, t = (C.c_int64 * 3)(), (C.c_int * 3)()
    m, b = (C.c_int * 3)(), (C.c_int * 3)()
    fb, fs = C.c_int(), C.c_int64()
    _check(_lib.spmv_spgemm_shape(e, t, m, b, C.byref(fb), C.byref(fs)),
           "spmv_spgemm_shape")
    return dict(edges=list(e), tables=list(t), teams=list(m),
                lds_bytes=list(b), fallback_batch=fb.value,
                fallback_bytes=fs.value)


#: CsrDevice.add_info of an add() result
AddResult = collections.namedtuple("AddResult",
                                   "nz matched widest rows_in_bin")


def add_shape():
    """the constants of CsrDevice.add() (host, no device): dict(edge, widths,
    threads) -- a row with len_A + len_B <= edge is served by a group of
    lanes, its width the smallest of widths that is not below the mean
    (NZ_A + NZ_B) / M, a longer one by a workgroup of `threads` lanes"""
    e, w = C.c_int64(), (C.c_int * 8)()
    n, t = C.c_int(), C.c_int()
    _check(_lib.spmv_add_shape(C.byref(e), w, C.byref(n), C.byref(t)),
           "spmv_add_shape")
    return dict(edge=e.value, widths=list(w)[:n.value], threads=t.value)


def add_set_class(mode):
    """MEASUREMENT and tests: which size class serves the rows of every add()
    from now on -- 0 the rule, 1 lane groups, 2 a workgroup per row; the
    bytes of a sum are the same.  -> the previous mode"""
    return _check(_lib.spmv_add_set_class(int(mode)), "spmv_add_set_class")


def add_last_phases():
    """host-clock ms of the last successful add() of this process:
    dict(checks, count, fill)"""
    ms = (C.c_double * 3)()
    _lib.spmv_add_last_phases(ms)
    return dict(zip(("checks", "count", "fill"), ms))


def spgemm_last_phases():
    """host-clock ms of the last successful matmul() of this process:
    dict(bound, symbolic, numeric, fallback) -- checks and bounds; class
    lists and symbolic pass; scan, allocation and numeric pass; the part of
    the last two spent in the fallback's launches (a measurement aid)"""
    ms = (C.c_double * 4)()
    _lib.spmv_spgemm_last_phases(ms)
    return dict(zip(("bound", "symbolic", "numeric", "fallback"), ms))


def trsv_shape():
    """the constants of the triangular solve (host, no device):
    dict(group, small_rows, threads) -- `group` lanes and sum slots per row (a
    power of two, part of the result contract), a level of at most
    `small_rows` rows joins a one-workgroup chain launch of `threads` lanes"""
    g, r, t = C.c_int(), C.c_int(), C.c_int()
    _lib.spmv_trsv_shape(C.byref(g), C.byref(r), C.byref(t))
    return dict(group=g.value, small_rows=r.value, threads=t.value)


def version():
    return _lib.spmv_version().decode()


def build_flavour():
    """"product" or "ablations" (spmv_engine.h)"""
    return _lib.spmv_build_flavour().decode()


def ignored_releases():
    """releases the library ignored (double release / stale wrapper): 0 in a
    correct program.  SPMV_DEBUG=1 prints one stderr line per occurrence."""
    return _lib.spmv_ignored_releases()


if os.environ.get("SPMV_DEBUG", "") not in ("", "0"):
    _lib.spmv_set_debug(1)


def seam_cache(level):
    """opt-in "keep the last upload" behind the one-shot seam (hip_csr.h):
    0 off (default, releases what is held), 1 matrix, 2 matrix + x (sampled
    fingerprints: the caller promises not to edit in place), 3 matrix + x
    with a full 64-bit hash of every byte per call (cannot be stale)"""
    _lib.spmv_seam_cache(int(level))


def seam_cache_invalidate(obj=None):
    """drop the cached copy of a matrix (sparse_csr / sparse_hll pointer),
    mark an uploaded x (numpy array) stale, or -- None -- drop everything
    held; -> slots touched (hip_csr.h: for callers that edit in place under
    levels 1 / 2)"""
    if obj is None:
        p = None
    elif isinstance(obj, np.ndarray):
        p = C.c_void_p(obj.ctypes.data)
    else:
        p = C.cast(obj, C.c_void_p)
    return _lib.spmv_seam_cache_invalidate(p)


def seam_cache_stats():
    """-> (matrices held, hits, misses)"""
    h, m = C.c_long(), C.c_long()
    held = _lib.spmv_seam_cache_stats(C.byref(h), C.byref(m))
    return held, h.value, m.value


def device_count():
    _check_the_hip_version_once()
    return _lib.spmv_device_count()


def device_pci_bus_id(device):
    buf = C.create_string_buffer(32)
    _check(_lib.spmv_device_pci_bus_id(device, buf, 32),
           "spmv_device_pci_bus_id")
    return buf.value.decode()


def rccl_version():
    """RCCL linked into the product library, as "2.22.3" (ncclGetVersion)"""
    v = _lib.spmv_mgpu_rccl_version()
    if v < 0:
        return None
    return "%d.%d.%d" % (v // 10000, v // 100 % 100, v % 100)


def set_device(d):
    _check(_lib.spmv_set_device(d), "spmv_set_device")


PANEL_SCHED = {"steps": 0, "sweep": 1, "chain": 2}


def set_panel_schedule(sched):
    """schedule the next build_panels() calls prepare (spmv_engine.h):
    "steps" / "sweep" / "chain", or 0 / 1 / 2 (True = sweep, False = steps)"""
    code = PANEL_SCHED[sched] if sched in PANEL_SCHED else int(sched)
    _check(_lib.spmv_set_panel_schedule(code), "spmv_set_panel_schedule")


def _env_int(name, lo, hi):
    try:
        v = int(os.environ.get(name, "0"))
    except ValueError:
        return 0
    return v if lo <= v <= hi else 0


_PIN_FIELDS = ("sched", "panel_cols", "tile_rows", "sweep_wgs_per_cu",
               "reserve_cus", "lds_min", "tile_order", "sweep_layout",
               "bucket_order", "deterministic")


def _layout_pin(fn_layout, h, chunk_fit=0):
    """the blocked copy's layout as one string, "sched=2,tile_rows=4096,...,
    waves=16" (None when there is no copy): what `build_panels_pinned` takes.
    chunk_fit=1 is appended for a sweep copy that carries its counted steps
    (panels_fit_steps): a string without it rebuilds a copy that launches the
    built-in shape, as every string written before the count existed"""
    o, w = PanelOpts(), C.c_int()
    o.struct_size = C.sizeof(PanelOpts)
    rc = fn_layout(h, C.byref(o), C.byref(w))
    if rc == -2:  # -ENOENT
        return None
    _check(rc, "spmv_*_panels_layout")
    return ",".join(["%s=%d" % (f, getattr(o, f)) for f in _PIN_FIELDS]
                    + ["waves=%d" % w.value]
                    + (["chunk_fit=1"] if chunk_fit else []))


def _pinned_opts(pin):
    """-> (PanelOpts, waves, chunk_fit) of a `panels_pin()` string; unknown
    keys are an error (a pin of another library version must not half-apply)"""
    o = PanelOpts()
    _lib.spmv_panel_opts_default(C.byref(o))
    waves = chunk_fit = 0
    for kv in pin.split(","):
        k, v = kv.split("=")
        if k == "waves":
            waves = int(v)
        elif k == "chunk_fit":
            chunk_fit = int(v)
        elif k in _PIN_FIELDS:
            setattr(o, k, int(v))
        else:
            raise ValueError("unknown field %r in blocked-layout pin" % k)
    return o, waves, chunk_fit


def _panel_opts(panel_cols=0, sched=None, tile_rows=0, sweep_wgs_per_cu=0,
                reserve_cus=0, lds_min=0, sweep_layout=None,
                deterministic=None):
    o = PanelOpts()
    _lib.spmv_panel_opts_default(C.byref(o))  # struct_size, the -1 defaults
    assert o.struct_size == C.sizeof(PanelOpts), "spmv_panel_opts ABI drift"
    o.sched = -1 if sched is None else (
        PANEL_SCHED[sched] if sched in PANEL_SCHED else int(sched))
    o.panel_cols = panel_cols
    o.tile_rows = tile_rows or _env_int("SPMV_TILE_ROWS", 32, 20448)
    o.sweep_wgs_per_cu = sweep_wgs_per_cu or _env_int("SPMV_SWEEP_WGS", 1, 8)
    o.reserve_cus = reserve_cus
    o.lds_min = lds_min or _env_int("SPMV_LDS_MIN", 1, 160 * 1024 - 256)
    if sweep_layout is None:  # -1: the library's default (panel-major)
        ev = os.environ.get("SPMV_SWEEP_LAYOUT", "")
        sweep_layout = int(ev) if ev in ("0", "1") else -1
    o.sweep_layout = sweep_layout
    o.bucket_order = _env_int("SPMV_BUCKET_ORDER", 0, 1)
    # None: the library's default (on for sweep layouts, off for chain /
    # steps); True / False: forced on / off (spmv_engine.h: 1 / 2)
    o.deterministic = 0 if deterministic is None else (1 if deterministic
                                                       else 2)
    return o


def dev_mem_info():
    """(free, total) bytes of HBM on the current device"""
    f, t = C.c_size_t(), C.c_size_t()
    _check(_lib.spmv_dev_mem_info(C.byref(f), C.byref(t)), "spmv_dev_mem_info")
    return f.value, t.value


def device_info(d=0):
    name = C.create_string_buffer(256)
    cus = C.c_int()
    mem = C.c_size_t()
    _check(_lib.spmv_device_info(d, name, 256, C.byref(cus), C.byref(mem)),
           "spmv_device_info")
    return name.value.decode(), cus.value, mem.value


# ---------------------------------------------------------------- CSR / HLL
_keepalive = {}


def io_load_csr(path):
    return _ptr_or_raise(_lib.io_load_csr(os.fsencode(path)), "io_load_csr")


def io_load_csr_cached(path):
    return _ptr_or_raise(_lib.io_load_csr_cached(os.fsencode(path)),
                         "io_load_csr_cached")


def csr_save_bin(A, path):
    _check(_lib.csr_save_bin(A, os.fsencode(path)), "csr_save_bin")


def csr_load_bin(path):
    return _ptr_or_raise(_lib.csr_load_bin(os.fsencode(path)), "csr_load_bin")


def csr_free(A):
    key = C.addressof(A.contents)
    if key in _keepalive:  # built over numpy arrays: nothing to free in C
        del _keepalive[key]
    else:
        _lib.csr_free(A)


def csr_from_arrays(name, M, N, IRP, JA, AS):
    """A sparse_csr whose arrays are the given numpy arrays (no copy when
    they are already int32 / float64 contiguous)."""
    IRP = np.ascontiguousarray(IRP, dtype=np.int32)
    JA = np.ascontiguousarray(JA, dtype=np.int32)
    AS = np.ascontiguousarray(AS, dtype=np.float64)
    assert len(IRP) == M + 1 and len(JA) == len(AS) == IRP[-1]
    s = SparseCSR()
    s.name = name.encode()[:MAX_NAME - 1]
    s.M, s.N, s.NZ = M, N, int(IRP[-1])
    s.IRP = IRP.ctypes.data_as(_ip)
    s.JA = JA.ctypes.data_as(_ip)
    s.AS = AS.ctypes.data_as(_dp)
    p = C.pointer(s)
    _keepalive[C.addressof(s)] = (s, IRP, JA, AS)
    return p


def csr_generate(kind, M, N, K, W, row0=0, seed=42):
    return _ptr_or_raise(_lib.csr_generate(kind, M, N, K, W, row0, seed),
                         "csr_generate")


def csr_row_slice(A, r0, r1):
    return _ptr_or_raise(_lib.csr_row_slice(A, r0, r1), "csr_row_slice")


def csr_arrays(A):
    """numpy views (no copy) of IRP, JA, AS."""
    a = A.contents
    IRP = np.ctypeslib.as_array(a.IRP, (a.M + 1,))
    JA = np.ctypeslib.as_array(a.JA, (max(a.NZ, 1),))[:a.NZ]
    AS = np.ctypeslib.as_array(a.AS, (max(a.NZ, 1),))[:a.NZ]
    return IRP, JA, AS


def extract_matrix_name(path):
    buf = C.create_string_buffer(MAX_NAME)
    _lib.extract_matrix_name(os.fsencode(path), buf)
    return buf.value.decode()


def partition_rows_nnz(A, parts):
    n = C.c_int(parts)
    p = _ptr_or_raise(_lib.partition_rows_nnz(A, C.byref(n)),
                      "partition_rows_nnz")
    out = np.ctypeslib.as_array(p, (n.value + 1,)).copy()
    _libc_free(p)
    return out


def partition_rows_even(M, parts, align=HACK_SIZE):
    p = _ptr_or_raise(_lib.partition_rows_even(M, parts, align),
                      "partition_rows_even")
    out = np.ctypeslib.as_array(p, (parts + 1,)).copy()
    _libc_free(p)
    return out


def partition_rows_nnz_aligned(IRP, parts, align=HACK_SIZE):
    """multi-GPU nnz-balanced cut (csr.h): starts[parts+1], boundaries
    multiples of `align`; IRP = the whole matrix's row offsets (or a
    sparse_csr pointer)"""
    if isinstance(IRP, _CSRp):
        M, irp = IRP.contents.M, IRP.contents.IRP
    else:
        IRP = np.ascontiguousarray(IRP, dtype=np.int32)
        M, irp = len(IRP) - 1, IRP.ctypes.data_as(_ip)
    p = _ptr_or_raise(_lib.partition_rows_nnz_aligned(irp, M, parts, align),
                      "partition_rows_nnz_aligned")
    out = np.ctypeslib.as_array(p, (parts + 1,)).copy()
    _libc_free(p)
    return out


def partition_synth_rows_nnz(kind, M, N, K, W, seed, parts, align=HACK_SIZE):
    """the same cut from a synthetic family's row lengths (no matrix built)"""
    p = _ptr_or_raise(
        _lib.partition_synth_rows_nnz(kind, M, N, K, W, seed, parts, align),
        "partition_synth_rows_nnz")
    out = np.ctypeslib.as_array(p, (parts + 1,)).copy()
    _libc_free(p)
    return out


_libc = C.CDLL(None)
_libc.free.argtypes = [C.c_void_p]


def _libc_free(p):
    _libc.free(C.cast(p, C.c_void_p))


def csr_to_hll(A, col_major):
    return _ptr_or_raise(_lib.csr_to_hll(A, bool(col_major)), "csr_to_hll")


def hll_free(H):
    _lib.hll_free(H)


def hll_num_slots(H):
    return _lib.hll_num_slots(H)


def hll_blocks(H):
    """list of (M, N, NZ, max_NZ, JA copy, AS copy) per hack block."""
    h = H.contents
    out = []
    for b in range(h.num_blocks):
        k = h.blocks[b]
        n = k.M * k.max_NZ
        ja = np.ctypeslib.as_array(k.JA, (n,)).copy() if n else np.zeros(0, np.int32)
        as_ = np.ctypeslib.as_array(k.AS, (n,)).copy() if n else np.zeros(0)
        out.append((k.M, k.N, k.NZ, k.max_NZ, ja, as_))
    return out


# ---------------------------------------------------------------- CPU benches
def bench_csr_serial(A, x):
    x, xp = _as_d(x)
    b = Bench()
    _check(_lib.bench_csr_serial(A, xp, C.byref(b)), "bench_csr_serial")
    return _take_vec(b.data), b.duration_ms, b.gflops


def _omp(fn, M, x, threads):
    x, xp = _as_d(x)
    b = BenchOmp()
    b.num_threads = threads
    _check(fn(M, xp, C.byref(b)), fn.__name__)
    return (_take_vec(b.bench.data), b.bench.duration_ms, b.bench.gflops,
            b.name.decode(), b.num_threads)


def bench_csr_omp_guided(A, x, threads):
    return _omp(_lib.bench_csr_omp_guided, A, x, threads)


def bench_csr_omp_nnz_balancing(A, x, threads):
    return _omp(_lib.bench_csr_omp_nnz_balancing, A, x, threads)


def bench_hll_serial(H, x, col_major=False):
    x, xp = _as_d(x)
    b = Bench()
    fn = _lib.bench_hll_serial_col_major if col_major else _lib.bench_hll_serial
    _check(fn(H, xp, C.byref(b)), "bench_hll_serial")
    return _take_vec(b.data), b.duration_ms, b.gflops


def bench_hll_omp(H, x, threads):
    return _omp(_lib.bench_hll_omp, H, x, threads)


def validation_vec_result(expected, res):
    e, ep = _as_d(expected)
    r, rp = _as_d(res)
    return _lib.validation_vec_result(Vec(len(e), ep), Vec(len(r), rp))


def max_rel_err(expected, res, scale=None):
    e, ep = _as_d(expected)
    r, rp = _as_d(res)
    sp = None
    if scale is not None:
        s, sp = _as_d(scale)
    return _lib.max_rel_err(Vec(len(e), ep), Vec(len(r), rp), sp)


# ---------------------------------------------------------------- GPU one-shot
def csr_spmv_hip(A, x, kernel=2, waves_per_block=0, group=0, variant=0):
    """y = A x through the one-shot C-ABI entry point (hip_csr.h): host
    arrays in, host y out, returns (y, kernel_ms)."""
    x, xp = _as_d(x)
    assert len(x) == A.contents.N
    y = np.zeros(A.contents.M)
    o = _opts(waves_per_block, group, variant)
    fn = getattr(_lib, "csr_spmv_hip_" + CSR_KERNEL_NAMES[kernel])
    ms = fn(A, xp, y.ctypes.data_as(_dp), C.cast(C.pointer(o), C.c_void_p))
    if ms < 0:
        _check(int(ms), "csr_spmv_hip_" + CSR_KERNEL_NAMES[kernel])
    return y, ms


def hll_spmv_hip(H, x, kernel=1, waves_per_block=0):
    x, xp = _as_d(x)
    assert len(x) == H.contents.N
    y = np.zeros(H.contents.M)
    o = _opts(waves_per_block)
    fn = getattr(_lib, "hll_spmv_hip_" + HLL_KERNEL_NAMES[kernel])
    ms = fn(H, xp, y.ctypes.data_as(_dp), C.cast(C.pointer(o), C.c_void_p))
    if ms < 0:
        _check(int(ms), "hll_spmv_hip_" + HLL_KERNEL_NAMES[kernel])
    return y, ms


def bench_csr_hip(A, x, kernel, waves_per_block=4):
    x, xp = _as_d(x)
    b = BenchHip()
    b.waves_per_block = waves_per_block
    fn = getattr(_lib, "bench_csr_hip_" + CSR_KERNEL_NAMES[kernel])
    _check(fn(A, xp, C.byref(b)), "bench_csr_hip_" + CSR_KERNEL_NAMES[kernel])
    return _take_vec(b.bench.data), b.bench.duration_ms, b.bench.gflops


def bench_hll_hip(H, x, kernel, waves_per_block=4):
    x, xp = _as_d(x)
    b = BenchHip()
    b.waves_per_block = waves_per_block
    fn = getattr(_lib, "bench_hll_hip_" + HLL_KERNEL_NAMES[kernel])
    _check(fn(H, xp, C.byref(b)), "bench_hll_hip_" + HLL_KERNEL_NAMES[kernel])
    return _take_vec(b.bench.data), b.bench.duration_ms, b.bench.gflops


# ---------------------------------------------------------------- persistent
# Lifetime of device objects.  Every DevBuffer / CsrDevice / HllDevice /
# MultiGpu is entered in `_live` (weak references).  Objects still alive when
# the interpreter exits -- a failed test's traceback holds its locals until
# then -- are NOT left to `__del__` during interpreter finalisation, where
# module globals are being cleared in no particular order: an atexit hook
# releases them first, in dependency order (multi-GPU handles with their
# communicators, then matrices, then raw buffers), while the runtime is fully
# up; afterwards `_closed` is set and every finaliser is a no-op.  Handles are
# released with the generation they were created with
# (spmv_*_release_checked): a second release, or a stale wrapper whose
# address the allocator reused, is ignored by the library and COUNTED
# (ignored_releases()).  (This ordering was built in round 3 against the exit
# abort of round 2; the abort's actual cause was the RTLD_GLOBAL load at the
# top of this file -- the ordered release stays because it is the right
# lifetime rule, not because it fixed that.)
_live = weakref.WeakSet()
_closed = False


def live_objects():
    """device objects created through this module and not yet released"""
    return [o for o in list(_live) if not o._released()]


def release_all():
    """release every live device object, dependents first; idempotent"""
    objs = live_objects()
    for cls_rank in (2, 1, 0):
        for o in objs:
            if o._RANK == cls_rank:
                try:
                    o._release_now()
                except Exception:  # noqa: BLE001 - keep releasing the rest
                    pass


def _at_exit():
    global _closed
    try:
        release_all()
    finally:
        _closed = True


atexit.register(_at_exit)


class DevBuffer:
    """Raw device allocation (for hosts that do not bring torch tensors)."""

    ptr = None
    _RANK = 0

    def __init__(self, nbytes):
        p = C.c_void_p()
        _check(_lib.spmv_dev_malloc(C.byref(p), nbytes), "spmv_dev_malloc")
        self.ptr, self.nbytes = p.value, nbytes
        _live.add(self)

    def _released(self):
        return not self.ptr

    def _release_now(self):
        self.free()

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        buf = cls(max(a.nbytes, 16))
        _check(_lib.spmv_copy_h2d(buf.ptr, a.ctypes.data, a.nbytes),
               "spmv_copy_h2d")
        return buf

    def to_numpy(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        _check(_lib.spmv_copy_d2h(out.ctypes.data, self.ptr, out.nbytes),
               "spmv_copy_d2h")
        return out

    def free(self):
        ptr, self.ptr = self.ptr, None
        if ptr and _closed is False and _lib is not None:
            _lib.spmv_dev_free(ptr)

    def __del__(self):
        if _closed is False:  # None / True at or after interpreter shutdown
            self.free()


def dev_fill_synth(ptr, n, seed, first=0, stream=None):
    _check(_lib.spmv_dev_fill_synth(ptr, n, seed, first, stream),
           "spmv_dev_fill_synth")


def device_sync():
    _check(_lib.spmv_device_sync(), "spmv_device_sync")


class Event:
    """GPU timer event (spmv_engine.h spmv_event_*; reference cuda_timer.cu):
    record() on a stream, a.elapsed_ms(b) waits for b"""

    def __init__(self):
        h = C.c_void_p()
        _check(_lib.spmv_event_create(C.byref(h)), "spmv_event_create")
        self.h = h

    def record(self, stream=None):
        _check(_lib.spmv_event_record(self.h, stream), "spmv_event_record")

    def elapsed_ms(self, stop):
        ms = C.c_float()
        _check(_lib.spmv_event_elapsed_ms(self.h, stop.h, C.byref(ms)),
               "spmv_event_elapsed_ms")
        return float(ms.value)

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h and _closed is False and _lib is not None:
            _lib.spmv_event_destroy(h)


class Stream:
    """a non-blocking HIP stream (spmv_stream_create); .ptr goes wherever a
    launch takes `stream`"""

    def __init__(self):
        h = C.c_void_p()
        _check(_lib.spmv_stream_create(C.byref(h)), "spmv_stream_create")
        self.ptr = h

    def sync(self):
        stream_sync(self.ptr)

    def capture(self, shape=False):
        """context manager: what is enqueued on this stream inside becomes a
        Graph (`with st.capture() as g: ...; g.launch()`).  shape=True: g.shape
        is dict(nodes, edges, roots, max_fanout) of what was captured -- a
        single chain has nodes - 1 edges, one root and max_fanout 1"""
        return _Capture(self, shape)

    def __del__(self):
        h, self.ptr = getattr(self, "ptr", None), None
        if h and _closed is False and _lib is not None:
            _lib.spmv_stream_destroy(h)


class Graph:
    """an instantiated hipGraph of captured launches (spmv_graph_*)"""
    h = None

    def launch(self, stream=None):
        _check(_lib.spmv_graph_launch(self.h, stream), "spmv_graph_launch")

    def destroy(self):
        h, self.h = self.h, None
        if h and _closed is False and _lib is not None:
            _lib.spmv_graph_destroy(h)

    def __del__(self):
        self.destroy()


class _Capture:
    def __init__(self, stream, shape=False):
        self.stream, self.graph, self.shape = stream, Graph(), shape

    def __enter__(self):
        _check(_lib.spmv_graph_begin_capture(self.stream.ptr),
               "spmv_graph_begin_capture")
        return self.graph

    def __exit__(self, et, ev, tb):
        h = C.c_void_p()
        if self.shape:
            n, e, r, f = C.c_int(), C.c_int(), C.c_int(), C.c_int()
            rc = _lib.spmv_graph_end_capture_shape(
                self.stream.ptr, C.byref(h), C.byref(n), C.byref(e),
                C.byref(r), C.byref(f))
            self.graph.shape = dict(nodes=n.value, edges=e.value,
                                    roots=r.value, max_fanout=f.value)
        else:
            rc = _lib.spmv_graph_end_capture(self.stream.ptr, C.byref(h))
        if et is None:
            _check(rc, "spmv_graph_end_capture")
            self.graph.h = h
        return False


def stream_sync(stream=None):
    _check(_lib.spmv_stream_sync(stream), "spmv_stream_sync")


def _upload_fn(fmt, values):
    if values not in ("f64", "f32"):
        raise ValueError("values=%r: \"f64\" or \"f32\"" % (values,))
    return "spmv_%s_upload%s" % (fmt, "_f32" if values == "f32" else "")


class _Device:
    """What CsrDevice and HllDevice share: the handle's lifecycle and the
    spmv_<fmt>_* calls that differ only in the prefix."""

    h = None
    _RANK = 1
    _FMT = None        # "csr" / "hll"
    _NUM_KERNELS = 0   # kernel ids of tune_times

    def __init__(self, handle):
        self.h = handle
        # the generation the library gave this handle: release_checked() acts
        # only on THAT handle, never on a newer one at a recycled address
        self.gen = _lib.spmv_handle_generation(self.h)
        if not self.gen:  # not a live handle: release_checked would be a
            #               silent no-op and the device memory would leak
            raise OSError(9, "spmv_handle_generation: %r is not a live "
                             "handle of this library" % (self.h,))
        self._read_shape()
        _live.add(self)

    def _released(self):
        return not self.h

    def _release_now(self):
        self.release()

    def _fn(self, name):
        return getattr(_lib, "spmv_%s_%s" % (self._FMT, name))

    def _call(self, name, *args):
        return _check(self._fn(name)(self.h, *args),
                      "spmv_%s_%s" % (self._FMT, name))

    @property
    def algorithmic_bytes(self):
        return self._fn("algorithmic_bytes")(self.h)

    @property
    def value_bytes(self):
        """8 (fp64 values) or 4 (stored as fp32; products and sums stay
        fp64)"""
        return self._call("value_bytes")

    def launch_multi(self, d_X, d_Y, k, ldx=0, ldy=0, waves_per_block=0,
                     group=0, stream=None):
        """Y[r*ldy + j] = sum_c A[r][c] * X[c*ldx + j] for j < k, 1 <= k <= 8
        vectors stored interleaved (ldx, ldy >= k; 0 = k): the matrix is read
        once for all k products.  Column j has the bits of launch(2, group)
        (CSR) / launch(1) (HLL, column-major only) on X[:, j].  X and Y must
        not overlap; only k columns of a row of Y are written.  `group` is
        ignored by HLL."""
        k, ldx, ldy = int(k), int(ldx), int(ldy)
        if not 1 <= k <= 8:
            raise ValueError("k=%r: 1..8 vectors per launch" % (k,))
        if (ldx and ldx < k) or (ldy and ldy < k):
            raise ValueError("ldx=%d, ldy=%d: at least k=%d (or 0)"
                             % (ldx, ldy, k))
        o = _opts(waves_per_block, group if self._FMT == "csr" else 0)
        self._call("launch_multi", C.byref(o), k, d_X, ldx, d_Y, ldy, stream)

    def multi_bytes(self, k):
        """bytes one launch_multi(k) must move: the matrix once, k vectors
        read and k written"""
        return _check(self._fn("multi_bytes")(self.h, int(k)),
                      "spmv_%s_multi_bytes" % self._FMT)

    def launch_axpby(self, alpha, beta, d_X, d_Y, k=1, ldx=0, ldy=0,
                     waves_per_block=0, group=0, stream=None):
        """Y = alpha * A X + beta * Y in place, layout and launch shape as
        launch_multi (k = 1..8 interleaved vectors, ldx, ldy >= k or 0).  With
        s what launch_multi stores: beta == 0 gives rn(alpha*s) and never
        reads Y (NaN, inf or uninitialised memory in it do not matter), else
        rn(rn(alpha*s) + rn(beta*y_old)) -- each operation rounded once, as
        the numpy expression alpha*S + beta*Y does.  alpha == 0 still reads
        the matrix (0 * NaN is NaN).  X and Y must not overlap.  A captured
        graph keeps the alpha and beta it was captured with."""
        k, ldx, ldy = int(k), int(ldx), int(ldy)
        if not 1 <= k <= 8:
            raise ValueError("k=%r: 1..8 vectors per launch" % (k,))
        if (ldx and ldx < k) or (ldy and ldy < k):
            raise ValueError("ldx=%d, ldy=%d: at least k=%d (or 0)"
                             % (ldx, ldy, k))
        o = _opts(waves_per_block, group if self._FMT == "csr" else 0)
        self._call("launch_axpby", C.byref(o), k, float(alpha), float(beta),
                   d_X, ldx, d_Y, ldy, stream)

    def axpby_bytes(self, k, beta):
        """bytes one launch_axpby(k) must move: multi_bytes(k), and Y once
        more (8*k*M) when beta != 0"""
        return _check(self._fn("axpby_bytes")(self.h, int(k),
                                              int(float(beta) != 0.0)),
                      "spmv_%s_axpby_bytes" % self._FMT)

    def cg(self, d_B, d_X, k=1, tol=1e-8, maxit=1000, check_every=0, ldb=0,
           ldx=0, work=None, waves_per_block=0, group=0, stream=None):
        """Conjugate gradients for A X = B on the device, A symmetric positive
        definite, k = 1..8 independent systems stored interleaved as in
        launch_multi (ldb, ldx >= k or 0).  d_X holds the initial guess and
        receives the iterate; d_B is not written.  Stops a column when
        r.r <= tol^2 b.b, after maxit iterations, or on a breakdown (p.Ap not
        positive, a non-finite scalar).  The call BLOCKS (it synchronises
        `stream` every check_every iterations, 0 = 8) and cannot be captured
        into a graph.  `work`: a DevBuffer of at least cg_work_bytes(M, k)
        bytes to solve without an allocation, None to let the library
        allocate and free one.  -> [CgResult(status, iterations, rr, bb)] * k;
        the result does not depend on check_every, work or waves_per_block."""
        return self._cg("cg", d_B, d_X, (), k, tol, maxit, check_every, ldb,
                        ldx, work, waves_per_block, group, stream)

    def pcg(self, d_B, d_X, d_minv, k=1, tol=1e-8, maxit=1000, check_every=0,
            ldb=0, ldx=0, work=None, waves_per_block=0, group=0, stream=None):
        """cg() preconditioned with z_i = minv_i * r_i: d_minv holds M
        doubles, one per row, shared by the k columns and never written.  Any
        positive vector; diag(d_minv, invert=True) gives Jacobi.  Everything
        else as cg() (`work`: at least pcg_work_bytes(M, k) bytes); a vector
        of ones returns the bits of cg().  A column whose r.z is not positive
        is a breakdown.  -> [CgResult(status, iterations, rr, bb)] * k"""
        return self._cg("pcg", d_B, d_X, (d_minv,), k, tol, maxit,
                        check_every, ldb, ldx, work, waves_per_block, group,
                        stream)

    def pcg_trsv(self, d_B, d_X, first, second=None, d_scale=None, k=1,
                 tol=1e-8, maxit=1000, check_every=0, ldb=0, ldx=0, work=None,
                 waves_per_block=0, group=0, stream=None):
        """cg() preconditioned by triangular plans: z = M^-1 r is
        first.solve(r -> z), then, with a second TrsvPlan,
        second.solve(z -> z in place, scale=d_scale).  Symmetric Gauss-Seidel:
        pcg_trsv(d_B, d_X, *A.sgs().args); IC(0): the lower plan of
        L = A.ic0()[0] and the upper plan of L.transpose().  The plans and
        d_scale (M doubles) are not written and may be shared by any number of
        solves.  Everything else as pcg() (`work`: at least
        pcg_trsv_work_bytes(M, k) bytes).  Each iteration adds the launches
        of the plans (TrsvPlan.info["launches"]).
        -> [CgResult(status, iterations, rr, bb)] * k"""
        if not isinstance(first, TrsvPlan) or \
                not (second is None or isinstance(second, TrsvPlan)):
            raise ValueError("pcg_trsv: first is a TrsvPlan, second a "
                             "TrsvPlan or None")
        if d_scale is not None and second is None:
            raise ValueError("pcg_trsv: d_scale scales the input of the "
                             "second plan, and there is none")
        return self._cg("pcg_trsv", d_B, d_X,
                        (first.h, second.h if second is not None else None,
                         d_scale), k, tol, maxit, check_every, ldb, ldx, work,
                        waves_per_block, group, stream)

    def pcg_amg(self, d_B, d_X, H, k=1, tol=1e-8, maxit=1000, check_every=0,
                ldb=0, ldx=0, work=None, waves_per_block=0, group=0,
                stream=None):
        """cg() preconditioned by one V cycle of an AmgHierarchy H
        (CsrDevice.amg() of a CSR handle of the same rows): pcg_trsv() word
        for word with Z = H.apply(R) where that has the plans' solves, k <=
        H.kmax (`work`: at least pcg_trsv_work_bytes(M, k) bytes).  H is not
        written and may serve any number of solves, one at a time.
        -> [CgResult(status, iterations, rr, bb)] * k"""
        if not isinstance(H, AmgHierarchy):
            raise ValueError("pcg_amg: H is an AmgHierarchy")
        return self._cg("pcg_amg", d_B, d_X, (H.h,), k, tol, maxit,
                        check_every, ldb, ldx, work, waves_per_block, group,
                        stream)

    def bicgstab(self, d_B, d_X, k=1, d_minv=None, tol=1e-8, maxit=1000,
                 check_every=0, ldb=0, ldx=0, work=None, waves_per_block=0,
                 group=0, stream=None):
        """BiCGStab for A X = B on the device, A square and otherwise
        arbitrary (nonsymmetric, indefinite): only A x is used, twice per
        iteration.  k, the layout, d_X / d_B, the blocking, check_every and
        `work` (at least bicgstab_work_bytes(M, k) bytes) as cg().  d_minv:
        M doubles of a right diagonal preconditioner (any sign;
        diag(d_minv, invert=True) gives Jacobi), never written; None: none,
        with the bits a vector of ones gives.  Stops a column when
        r.r <= tol^2 b.b, after maxit iterations, or on a breakdown (rh.v
        zero, a non-finite scalar).
        -> [CgResult(status, iterations, rr, bb)] * k"""
        return self._cg("bicgstab", d_B, d_X, (d_minv,), k, tol, maxit,
                        check_every, ldb, ldx, work, waves_per_block, group,
                        stream)

    def bicgstab_trsv(self, d_B, d_X, first, second=None, d_scale=None, k=1,
                      tol=1e-8, maxit=1000, check_every=0, ldb=0, ldx=0,
                      work=None, waves_per_block=0, group=0, stream=None):
        """bicgstab() with a right preconditioner made by triangular plans:
        z = M^-1 u is first.solve(u -> z), then, with a second TrsvPlan,
        second.solve(z -> z in place, scale=d_scale).  ILU(0): with
        LU = A.ilu0()[0], first = LU.trsv_analyse("lower", unit=True) and
        second = LU.trsv_analyse("upper"); symmetric Gauss-Seidel:
        bicgstab_trsv(d_B, d_X, *A.sgs().args).  The plans and d_scale (M
        doubles) are not written and may be shared by any number of solves.
        Everything else as bicgstab() (`work`: at least
        bicgstab_trsv_work_bytes(M, k) bytes).  Each iteration adds the
        launches of the plans twice (TrsvPlan.info["launches"]).
        -> [CgResult(status, iterations, rr, bb)] * k"""
        if not isinstance(first, TrsvPlan) or \
                not (second is None or isinstance(second, TrsvPlan)):
            raise ValueError("bicgstab_trsv: first is a TrsvPlan, second a "
                             "TrsvPlan or None")
        if d_scale is not None and second is None:
            raise ValueError("bicgstab_trsv: d_scale scales the input of the "
                             "second plan, and there is none")
        return self._cg("bicgstab_trsv", d_B, d_X,
                        (first.h, second.h if second is not None else None,
                         d_scale), k, tol, maxit, check_every, ldb, ldx, work,
                        waves_per_block, group, stream)

    def minres(self, d_B, d_X, k=1, d_minv=None, tol=1e-8, maxit=1000,
               check_every=0, ldb=0, ldx=0, work=None, waves_per_block=0,
               group=0, stream=None):
        """MINRES for A X = B on the device, A square and symmetric, definite
        or not (KKT and saddle-point matrices, shifted stencils; symmetry is
        not checked): one product per iteration and a residual estimate that
        never grows.  k, the layout, d_X / d_B, the blocking, check_every and
        `work` (at least minres_work_bytes(M, k) bytes) as cg().  d_minv: M
        doubles of a POSITIVE diagonal preconditioner, never written
        (diag(d_minv, invert=True) where the diagonal is positive; 1 / |d|
        with 1 where d == 0 for a saddle point); None: none, with the bits a
        vector of ones gives.  Stops a column when pp <= tol^2 bn2 -- pp the
        recurrence's squared residual estimate, bn2 = b.z(b), both in the
        norm of the preconditioner -- after maxit iterations, or on a
        breakdown (u.z(u) negative, a non-finite scalar, gamma == 0).  rr is
        the true r.r of b - A x, computed once at the end.
        -> [MinresResult(status, iterations, pp, bn2, rr, bb)] * k"""
        return self._cg("minres", d_B, d_X, (d_minv,), k, tol, maxit,
                        check_every, ldb, ldx, work, waves_per_block, group,
                        stream, MinresInfo, MinresResult)

    def gmres(self, d_B, d_X, k=1, restart=30, d_minv=None, tol=1e-8,
              maxit=1000, check_every=0, ldb=0, ldx=0, work=None,
              waves_per_block=0, group=0, stream=None):
        """Restarted GMRES(restart) for A X = B on the device, A square and
        otherwise arbitrary: one product and one preconditioner apply per
        Arnoldi step, a residual estimate that never grows within a cycle,
        and no breakdown other than a singular matrix or a non-finite number.
        restart = 1..64 steps per cycle; maxit counts steps over all cycles.
        k, the layout, d_X / d_B, d_minv (a right diagonal preconditioner or
        None), the blocking, check_every and `work` (at least
        gmres_work_bytes(M, k, restart) bytes) as bicgstab().  Stops a column
        when est <= tol^2 b.b -- est the recurrence's squared residual
        estimate; at a restart the true r.r -- after maxit steps, or on a
        breakdown.  rr is the true r.r of b - A x, computed once at the end.
        -> [GmresResult(status, iterations, restarts, rr, est, bb)] * k"""
        restart = self._restart(restart)
        return self._cg("gmres", d_B, d_X, (d_minv, restart), k, tol, maxit,
                        check_every, ldb, ldx, work, waves_per_block, group,
                        stream, GmresInfo, GmresResult)

    def gmres_trsv(self, d_B, d_X, first, second=None, d_scale=None, k=1,
                   restart=30, tol=1e-8, maxit=1000, check_every=0, ldb=0,
                   ldx=0, work=None, waves_per_block=0, group=0, stream=None):
        """gmres() with a right preconditioner made by triangular plans, as
        bicgstab_trsv(): ILU(0) is (LU.trsv_analyse("lower", unit=True),
        LU.trsv_analyse("upper")) of LU = A.ilu0()[0]; symmetric Gauss-Seidel
        is gmres_trsv(d_B, d_X, *A.sgs().args).  Each step adds the launches
        of the plans once (TrsvPlan.info["launches"]), where bicgstab_trsv()
        adds them twice per iteration.  `work`: at least
        gmres_work_bytes(M, k, restart) bytes.
        -> [GmresResult(status, iterations, restarts, rr, est, bb)] * k"""
        if not isinstance(first, TrsvPlan) or \
                not (second is None or isinstance(second, TrsvPlan)):
            raise ValueError("gmres_trsv: first is a TrsvPlan, second a "
                             "TrsvPlan or None")
        if d_scale is not None and second is None:
            raise ValueError("gmres_trsv: d_scale scales the input of the "
                             "second plan, and there is none")
        restart = self._restart(restart)
        return self._cg("gmres_trsv", d_B, d_X,
                        (first.h, second.h if second is not None else None,
                         d_scale, restart), k, tol, maxit, check_every, ldb,
                        ldx, work, waves_per_block, group, stream, GmresInfo,
                        GmresResult)

    @staticmethod
    def _restart(restart):
        restart = int(restart)
        if not 1 <= restart <= GMRES_MAX_RESTART:
            raise ValueError("restart=%r: 1..%d steps per cycle"
                             % (restart, GMRES_MAX_RESTART))
        return restart

    def _cg(self, name, d_B, d_X, minv, k, tol, maxit, check_every, ldb, ldx,
            work, waves_per_block, group, stream, record=CgInfo,
            result=CgResult):
        """cg(), pcg(), pcg_trsv(), bicgstab() and minres(): `minv` is () or
        (d_minv,) or (first, second, d_scale), the arguments spmv_*_cg does
        not take; `record` / `result`: the C
        record of the solver and the namedtuple with its fields"""
        k, ldb, ldx = int(k), int(ldb), int(ldx)
        if not 1 <= k <= 8:
            raise ValueError("k=%r: 1..8 systems per solve" % (k,))
        if (ldb and ldb < k) or (ldx and ldx < k):
            raise ValueError("ldb=%d, ldx=%d: at least k=%d (or 0)"
                             % (ldb, ldx, k))
        o = _opts(waves_per_block, group if self._FMT == "csr" else 0)
        info = (record * k)()
        self._call(name, C.byref(o), k, d_B, ldb, d_X, ldx, *minv, float(tol),
                   int(maxit), int(check_every),
                   work.ptr if work is not None else None,
                   work.nbytes if work is not None else 0, info, stream)
        return [result(*(getattr(i, f) for f in result._fields))
                for i in info]

    def cgls(self, dAT, d_B, d_X, k=1, damp=0.0, tol=1e-8, maxit=1000,
             check_every=0, ldb=0, ldx=0, work=None, waves_per_block=0,
             group=0, stream=None):
        """CGLS for min ||A X - B||^2 + damp^2 ||X||^2 on the device, A this
        M x N handle (any shape) and dAT its N x M transpose as a handle of
        the same class: transpose() for a CSR pair, transpose().to_hll(True)
        for an HLL pair.  That dAT is the transpose is not checked, only its
        shape.  d_B has M rows and d_X has N rows of k = 1..8 interleaved
        columns (ldb, ldx >= k or 0); d_X holds the initial guess (zero gives
        the minimum-norm solution of a wide A) and receives the iterate, d_B
        is not written.  Stops a column when s.s <= tol^2 (A^T b).(A^T b)
        with s = A^T r - damp^2 x, after maxit iterations, or on a breakdown
        (delta not positive, a non-finite scalar).  The blocking, check_every
        and `work` (at least cgls_work_bytes(M, N, k) bytes) as cg().
        -> [CglsResult(status, iterations, ss, atb, rr)] * k"""
        k, ldb, ldx = int(k), int(ldb), int(ldx)
        if not 1 <= k <= 8:
            raise ValueError("k=%r: 1..8 problems per solve" % (k,))
        if (ldb and ldb < k) or (ldx and ldx < k):
            raise ValueError("ldb=%d, ldx=%d: at least k=%d (or 0)"
                             % (ldb, ldx, k))
        if type(dAT) is not type(self):
            raise TypeError("cgls: the transpose must be a %s like the "
                            "matrix, not %r" % (type(self).__name__,
                                                type(dAT).__name__))
        o = _opts(waves_per_block, group if self._FMT == "csr" else 0)
        info = (CglsInfo * k)()
        self._call("cgls", dAT.h, C.byref(o), k, d_B, ldb, d_X, ldx,
                   float(damp), float(tol), int(maxit), int(check_every),
                   work.ptr if work is not None else None,
                   work.nbytes if work is not None else 0, info, stream)
        return [CglsResult(i.status, i.iterations, i.ss, i.atb, i.rr)
                for i in info]

    def diag(self, d_out, invert=False, stream=None):
        """d_out[r] = the fp64 sum of the stored entries of row r in column
        r, for r < min(M, N) (0.0 where the row stores none); invert=True
        stores 1.0 / that sum instead (inf for a zero diagonal): the Jacobi
        preconditioner of pcg().  Asynchronous on `stream`, capturable."""
        self._call("diag", d_out, int(bool(invert)), stream)

    def build_panels(self, panel_cols=0, sched=None, tile_rows=0,
                     sweep_wgs_per_cu=0, reserve_cus=0, lds_min=0,
                     sweep_layout=None, deterministic=None):
        """blocked copy in the process default schedule, or in an explicit
        one ("steps" / "sweep" / "chain"), with explicit build options
        (spmv_panel_opts).  The experiment knobs SPMV_TILE_ROWS,
        SPMV_SWEEP_WGS and SPMV_LDS_MIN of tools/README.md are read HERE, in
        the harness -- the library itself reads no environment."""
        o = _panel_opts(panel_cols, sched, tile_rows, sweep_wgs_per_cu,
                        reserve_cus, lds_min, sweep_layout, deterministic)
        self._call("build_panels_opts", C.byref(o))

    def panels_tile_rows(self):
        rc = self._fn("panels_tile_rows")(self.h)
        return None if rc < 0 else rc

    def panels_describe(self):
        """one line: schedule, geometry, bucket order, launch shape; None
        when no blocked copy is built"""
        buf = C.create_string_buffer(256)
        rc = self._fn("panels_describe")(self.h, buf, 256)
        return None if rc else buf.value.decode()

    def panels_pin(self):
        """the layout of the blocked copy (schedule, tile height, orders,
        waves) as a string that `build_panels_pinned` rebuilds exactly"""
        fit = self.panels_fit_steps() if self.panels_describe() else None
        return _layout_pin(self._fn("panels_layout"), self.h,
                           bool(fit and fit[0] > 0))

    def build_panels_pinned(self, pin):
        o, waves, chunk_fit = _pinned_opts(pin)
        self._call("build_panels_opts", C.byref(o))
        self._call("panels_set_waves", waves)
        if not chunk_fit:
            self.panels_set_fit_steps(0, 0)

    def panels_fit_steps(self):
        """sweep copy: (steps with the built-in shape's chunk, steps with the
        4608-slot chunk) counted at the build; (0, 0): not counted"""
        a, b = C.c_int64(), C.c_int64()
        self._call("panels_fit_steps", C.byref(a), C.byref(b))
        return a.value, b.value

    def panels_set_fit_steps(self, builtin, fit):
        """(0, 0): launch the built-in shape (a copy without the count)"""
        self._call("panels_set_fit_steps", builtin, fit)

    def panels_plan(self, waves_per_block=0, variant=0):
        """-> (threads, groups per lane, ordered) of the tile kernel a blocked
        launch with these options would run"""
        o = _opts(waves_per_block, 0, variant)
        t, q, d = C.c_int(), C.c_int(), C.c_int()
        self._call("panels_plan", C.byref(o), C.byref(t), C.byref(q),
                   C.byref(d))
        return t.value, q.value, d.value

    def build_panels_like(self, model):
        self._call("build_panels_like", model.h)

    def panels_schedule(self):
        """-> "steps" / "sweep" / "chain", or None when not built"""
        rc = self._fn("panels_schedule")(self.h)
        return None if rc < 0 else ("steps", "sweep", "chain")[rc]

    def release_source(self):
        """keep only the blocked copy (frees JA/AS on the device)"""
        self._call("release_source")

    def panels_info(self):
        """-> dict(steps, tiles, panels, entries) or None when not built"""
        a, b, c, n = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        rc = self._fn("panels_info")(self.h, C.byref(a), C.byref(b),
                                     C.byref(c), C.byref(n))
        return None if rc else dict(steps=a.value, tiles=b.value,
                                    panels=c.value, entries=n.value)

    def autotune(self, d_x, d_y, allow_panels=True):
        """-> (kernel id, median ms) of the fastest kernel for this matrix"""
        k, ms = C.c_int(), C.c_double()
        self._call("autotune", d_x, d_y, int(allow_panels), C.byref(k),
                   C.byref(ms))
        return k.value, ms.value

    def tune_times(self):
        """per-kernel median ms of the last autotune (0.0: not a candidate)"""
        ms = (C.c_double * self._NUM_KERNELS)()
        self._call("tune_times", ms, self._NUM_KERNELS)
        return list(ms)

    def tune_log(self):
        """what the last autotune did (text, one line per phase) or None"""
        buf = C.create_string_buffer(16384)
        rc = self._fn("tune_log")(self.h, buf, 16384)
        return None if rc else buf.value.decode()

    def release(self):
        h, self.h = self.h, None
        if h and _closed is False and _lib is not None:
            self._fn("release_checked")(h, self.gen)

    def __del__(self):
        if _closed is False:  # None / True at or after interpreter shutdown
            self.release()


class CsrDevice(_Device):
    """A CSR matrix resident in HBM (spmv_engine.h, spmv_csr_dev)."""

    _FMT = "csr"
    _NUM_KERNELS = NUM_CSR_KERNELS_ALL

    def _read_shape(self):
        M, N, NZ = C.c_int(), C.c_int(), C.c_int64()
        _check(_lib.spmv_csr_shape(self.h, C.byref(M), C.byref(N),
                                   C.byref(NZ)), "spmv_csr_shape")
        self.M, self.N, self.NZ = M.value, N.value, NZ.value

    @classmethod
    def upload(cls, A, values="f64"):
        """values="f32": the matrix values are rounded to fp32 and stored so
        (8 instead of 12 bytes per entry; OSError(ERANGE) when a finite value
        overflows); x, y, products and sums stay fp64"""
        name = _upload_fn("csr", values)
        h = C.c_void_p()
        _check(getattr(_lib, name)(A, C.byref(h)), name)
        return cls(h)

    def to_f32(self):
        """a new handle with this one's pattern and its values rounded to
        fp32 on the device; this handle stays valid"""
        h = C.c_void_p()
        _check(_lib.spmv_csr_to_f32(self.h, C.byref(h)), "spmv_csr_to_f32")
        return CsrDevice(h)

    def transpose(self):
        """a new N x M handle T = A^T built on the device: this handle's
        entries in the stable order by column (spmv_engine.h), the same value
        type; y = A^T x is a launch of T.  This handle stays valid"""
        h = C.c_void_p()
        _check(_lib.spmv_csr_transpose(self.h, C.byref(h)),
               "spmv_csr_transpose")
        return CsrDevice(h)

    def _product(self, h, info):
        d = CsrDevice(h)
        d.spgemm_info = SpgemmResult(info.products, info.widest,
                                     tuple(info.rows_in_bin), info.nz)
        return d

    def matmul(self, other):
        """a new M x N f64 handle C = self . other built on the device
        (spmv_engine.h, spmv_csr_spgemm): every column a product meets, once,
        ascending; each value the sequential sum of its products in the order
        of the walk over this handle's stored entries and other's rows, the
        first product initialising the sum, nothing fused -- defined to the
        bit.  Either operand may be f32-stored; `other` may be this handle.
        other's rows must be strictly ascending by column
        (OSError(EINVAL); transpose().transpose() sorts rows).  The result
        carries .spgemm_info (products, widest, rows_in_bin, nz).  Both
        operands stay valid"""
        if not isinstance(other, CsrDevice):
            raise TypeError("matmul: a CsrDevice, not %s"
                            % type(other).__name__)
        h, info = C.c_void_p(), SpgemmInfo()
        _check(_lib.spmv_csr_spgemm(self.h, other.h, C.byref(h),
                                    C.byref(info)), "spmv_csr_spgemm")
        return self._product(h, info)

    def add(self, other, alpha=1.0, beta=1.0):
        """a new M x N f64 handle C = alpha self + beta other built on the
        device (spmv_engine.h, spmv_csr_add): in every row the union of the
        two rows' columns, once each, ascending; rn(alpha a), rn(beta b), or
        the rounded sum of the two where both store the column, nothing
        fused -- defined to the byte.  Either operand may be f32-stored;
        `other` may be this handle.  The rows of both must be strictly
        ascending by column (OSError(EINVAL); transpose().transpose() sorts
        rows); alpha and beta must be finite.  The result carries .add_info
        (nz, matched, widest, rows_in_bin).  Both operands stay valid"""
        if not isinstance(other, CsrDevice):
            raise TypeError("add: a CsrDevice, not %s" % type(other).__name__)
        h, info = C.c_void_p(), AddInfo()
        _check(_lib.spmv_csr_add(float(alpha), self.h, float(beta), other.h,
                                 C.byref(h), C.byref(info)), "spmv_csr_add")
        d = CsrDevice(h)
        d.add_info = AddResult(info.nz, info.matched, info.widest,
                               tuple(info.rows_in_bin))
        return d

    @classmethod
    def from_diag(cls, M, d_diag=None):
        """a new M x M f64 handle with the one entry (i, i) per row: the bits
        of the M doubles at the device pointer d_diag, or 1.0 (the identity)
        when it is None (spmv_csr_from_diag)"""
        h = C.c_void_p()
        _check(_lib.spmv_csr_from_diag(int(M), d_diag, C.byref(h)),
               "spmv_csr_from_diag")
        return cls(h)

    def scale(self, d_left=None, d_right=None):
        """a new f64 handle with this one's pattern byte for byte and the
        values rn(rn(l_i a) r_j): d_left M and d_right N doubles on the
        device, either may be None but not both (spmv_csr_scale).  This
        handle may be f32-stored, of any shape, with unsorted rows and
        duplicates, and stays valid"""
        h = C.c_void_p()
        _check(_lib.spmv_csr_scale(self.h, d_left, d_right, C.byref(h)),
               "spmv_csr_scale")
        return CsrDevice(h)

    def galerkin(self, dP, dPT=None):
        """a new handle dPT . (self . dP): the coarse operator of a
        prolongation dP, two matmul() and nothing else (spmv_csr_galerkin).
        dPT None: dP.transpose(), built and released; the intermediate
        product is released.  .spgemm_info describes the second product"""
        for d in (dP,) + ((dPT,) if dPT is not None else ()):
            if not isinstance(d, CsrDevice):
                raise TypeError("galerkin: a CsrDevice, not %s"
                                % type(d).__name__)
        h, info = C.c_void_p(), SpgemmInfo()
        _check(_lib.spmv_csr_galerkin(self.h, dP.h,
                                      dPT.h if dPT is not None else None,
                                      C.byref(h), C.byref(info)),
               "spmv_csr_galerkin")
        return self._product(h, info)

    def symmetry(self):
        """SYM_NONE, SYM_PATTERN or SYM_VALUES: entries compared position by
        position after the stable ordering, duplicates not summed, values
        with == (a NaN is never symmetric)"""
        out = C.c_int()
        _check(_lib.spmv_csr_symmetry(self.h, C.byref(out)),
               "spmv_csr_symmetry")
        return out.value

    def trsv_analyse(self, uplo="lower", unit=False, max_levels=0, sweeps=0,
                     kmax=8):
        """a TrsvPlan for T x = b with T the `uplo` triangle of this (square)
        handle: the level schedule and a copy of the strict entries, built on
        the device and defined to the byte (spmv_engine.h).  unit=True: unit
        diagonal.  More than max_levels levels (0: 1 << 20) is
        OSError(E2BIG).  sweeps > 0 (up to 4096): a SWEEP PLAN instead -- the
        solve is that many Jacobi sweeps, one launch each, approximate below
        the depth of the triangle and exact to the bit from there on; no
        levels are computed, max_levels is ignored, and a solve takes at most
        kmax (1..8) right-hand sides.  Two solves of one sweep plan must not
        overlap in time (they share its scratch).  This handle stays valid
        and may be released"""
        if uplo not in ("lower", "upper"):
            raise ValueError("uplo=%r: \"lower\" or \"upper\"" % (uplo,))
        max_levels, sweeps, kmax = int(max_levels), int(sweeps), int(kmax)
        if max_levels < 0:
            raise ValueError("max_levels=%d: 0 (the default) or more"
                             % max_levels)
        if not 0 <= sweeps <= 4096:
            raise ValueError("sweeps=%d: 0 (an exact plan) or 1..4096"
                             % sweeps)
        if not 1 <= kmax <= 8:
            raise ValueError("kmax=%d: 1..8 right-hand sides" % kmax)
        h = C.c_void_p()
        if sweeps:
            _check(_lib.spmv_csr_trsv_analyse_sweeps(
                self.h, int(uplo == "upper"), int(bool(unit)), sweeps, kmax,
                C.byref(h)), "spmv_csr_trsv_analyse_sweeps")
            return TrsvPlan(h)
        _check(_lib.spmv_csr_trsv_analyse(self.h, int(uplo == "upper"),
                                          int(bool(unit)), max_levels,
                                          C.byref(h)),
               "spmv_csr_trsv_analyse")
        return TrsvPlan(h)

    def ic0(self, shift=0.0, max_levels=0):
        """(L, Ic0Info): the zero-fill incomplete Cholesky factor of this
        (square, f64) handle, A + shift diag(A) ~ L L^T, as a new CsrDevice
        with the pattern of the lower triangle, the diagonal last in each
        row, built on the device and defined to the bit (spmv_engine.h).
        Only entries with column <= row are read; they must be strictly
        ascending in every row and hold the diagonal (OSError(EINVAL)
        otherwise; transpose().transpose() sorts rows).  A pivot that is not
        positive is counted in Ic0Info.bad_pivots and leaves NaN in L, it is
        not an error.  The preconditioner of pcg_trsv() is
        (L.trsv_analyse("lower"), L.transpose().trsv_analyse("upper")).
        This handle stays valid"""
        shift, max_levels = float(shift), int(max_levels)
        if not (shift >= 0.0 and np.isfinite(shift)):
            raise ValueError("shift=%r: a finite number, 0 or more"
                             % (shift,))
        if max_levels < 0:
            raise ValueError("max_levels=%d: 0 (the default) or more"
                             % max_levels)
        h, info = C.c_void_p(), Ic0Info()
        _check(_lib.spmv_csr_ic0(self.h, shift, max_levels, C.byref(h),
                                 C.byref(info)), "spmv_csr_ic0")
        return CsrDevice(h), info

    def ilu0(self, shift=0.0, max_levels=0):
        """(LU, Ilu0Info): the zero-fill incomplete LU factors of this
        (square, f64) handle, A + shift diag(A) ~ L U, as ONE new CsrDevice
        with exactly this handle's pattern: L strictly below the diagonal
        (its unit diagonal implied), U on and above it, built on the device
        and defined to the bit (spmv_engine.h).  Every row must be strictly
        ascending and hold its diagonal (OSError(EINVAL) otherwise;
        transpose().transpose() sorts rows).  A pivot that is zero or not
        finite is counted in Ilu0Info.bad_pivots and leaves inf / NaN in the
        dependent rows, it is not an error.  The preconditioner of
        bicgstab_trsv() is (LU.trsv_analyse("lower", unit=True),
        LU.trsv_analyse("upper")).  This handle stays valid"""
        shift, max_levels = float(shift), int(max_levels)
        if not (shift >= 0.0 and np.isfinite(shift)):
            raise ValueError("shift=%r: a finite number, 0 or more"
                             % (shift,))
        if max_levels < 0:
            raise ValueError("max_levels=%d: 0 (the default) or more"
                             % max_levels)
        h, info = C.c_void_p(), Ilu0Info()
        _check(_lib.spmv_csr_ilu0(self.h, shift, max_levels, C.byref(h),
                                  C.byref(info)), "spmv_csr_ilu0")
        return CsrDevice(h), info

    def colour(self, seed=0, max_rounds=0):
        """a Colouring of this (square) handle: the deterministic first-fit
        colouring by the priority fmix32(row ^ seed) and the ordering that
        numbers the rows colour by colour, found on the device and defined to
        the byte (spmv_engine.h).  Only the pattern is read, through A and
        A^T.  More than max_rounds rounds (0: 4096) is OSError(E2BIG).
        permute(col, col) then has plans of at most col.colours levels"""
        seed, max_rounds = int(seed), int(max_rounds)
        if not 0 <= seed < 1 << 32:
            raise ValueError("seed=%d: a 32-bit unsigned number" % seed)
        if max_rounds < 0:
            raise ValueError("max_rounds=%d: 0 (the default) or more"
                             % max_rounds)
        return Colouring(self, seed, max_rounds)

    def permute(self, rows=None, cols=None):
        """a new CsrDevice B = P A Q^T: row r becomes row rows[r], column c
        becomes cols[c], every row stably sorted by new column, values moved
        with their bits (spmv_engine.h).  rows / cols: a DevBuffer of int32
        (M / N of them), a raw device pointer, a Colouring (its .perm) or
        None for the identity.  An array that is no permutation is
        OSError(EDOM) (an entry out of range) or OSError(EINVAL) (a repeated
        entry).  This handle stays valid"""
        h = C.c_void_p()
        _check(_lib.spmv_csr_permute(self.h, _perm_ptr(rows, "rows"),
                                     _perm_ptr(cols, "cols"), C.byref(h)),
               "spmv_csr_permute")
        return CsrDevice(h)

    def aggregate(self, theta=0.0, seed=0, max_rounds=0):
        """an Aggregation of this (square, f64) handle, rows strictly
        ascending with their diagonal: the roots are a distance-2 maximal
        independent set of the strength graph (entry (i, j) strong iff
        a_ij^2 >= theta^2 |d_i d_j|) found by parallel rounds with the
        priority fmix32(row ^ seed), every other row joins its strongest
        strong neighbour's aggregate -- defined to the integer
        (spmv_engine.h).  More than max_rounds rounds (0: 4096) is
        OSError(E2BIG)"""
        theta, seed, max_rounds = float(theta), int(seed), int(max_rounds)
        if not (theta >= 0.0 and np.isfinite(theta)):
            raise ValueError("theta=%r: a finite number, 0 or more" % (theta,))
        if not 0 <= seed < 1 << 32:
            raise ValueError("seed=%d: a 32-bit unsigned number" % seed)
        if max_rounds < 0:
            raise ValueError("max_rounds=%d: 0 (the default) or more"
                             % max_rounds)
        return Aggregation(self, theta, seed, max_rounds)

    def amg(self, theta=0.0, sweeps=1, coarse_sweeps=8, min_rows=32,
            max_levels=16, seed=0, kmax=8):
        """an AmgHierarchy of this (square, f64) handle: smoothed aggregation
        (aggregate(theta, seed), P = (I - 4/3 / rho D^-1 A) T, Galerkin
        products) down to a level of at most min_rows rows or max_levels
        levels, built on the device and defined to the bit (spmv_engine.h).
        Its cycle is V(sweeps, sweeps) with damped Jacobi and coarse_sweeps
        sweeps on the coarsest level, for at most kmax right-hand sides.  The
        hierarchy BORROWS this handle: keep it alive while the hierarchy is
        used"""
        theta = float(theta)
        sweeps, coarse_sweeps = int(sweeps), int(coarse_sweeps)
        min_rows, max_levels = int(min_rows), int(max_levels)
        seed, kmax = int(seed), int(kmax)
        if not (theta >= 0.0 and np.isfinite(theta)):
            raise ValueError("theta=%r: a finite number, 0 or more" % (theta,))
        if not (1 <= sweeps <= 64 and 1 <= coarse_sweeps <= 64):
            raise ValueError("sweeps=%d, coarse_sweeps=%d: 1..64"
                             % (sweeps, coarse_sweeps))
        if min_rows < 1 or not 1 <= max_levels <= AMG_MAX_LEVELS:
            raise ValueError("min_rows=%d (1 or more), max_levels=%d (1..%d)"
                             % (min_rows, max_levels, AMG_MAX_LEVELS))
        if not 0 <= seed < 1 << 32:
            raise ValueError("seed=%d: a 32-bit unsigned number" % seed)
        if not 1 <= kmax <= 8:
            raise ValueError("kmax=%d: 1..8 right-hand sides" % kmax)
        h = C.c_void_p()
        _check(_lib.spmv_csr_amg_setup(self.h, theta, sweeps, coarse_sweeps,
                                       min_rows, max_levels, seed, kmax,
                                       C.byref(h)), "spmv_csr_amg_setup")
        return AmgHierarchy(h, self)

    def sgs(self, max_levels=0, sweeps=0, kmax=8):
        """an SgsPreconditioner of this (square) handle: its lower and upper
        TrsvPlan and a DevBuffer with diag(A); release() frees the three.
        sweeps > 0: both are sweep plans of that many sweeps (trsv_analyse;
        the same count in both keeps the preconditioner symmetric)"""
        return SgsPreconditioner(self, max_levels, sweeps, kmax)

    @classmethod
    def generate(cls, kind, M, N, K, W, row0=0, seed=42):
        h = C.c_void_p()
        _check(_lib.spmv_csr_generate(kind, M, N, K, W, row0, seed,
                                      C.byref(h)), "spmv_csr_generate")
        return cls(h)

    def kernel_bytes(self, kernel):
        """CSR stores no padding: every kernel is priced on the same bytes"""
        return self.algorithmic_bytes

    def launch(self, kernel, d_x, d_y, waves_per_block=0, group=0,
               stream=None, rows=None, variant=0):
        o = _opts(waves_per_block, group, variant)
        if rows is None:
            rc = _lib.spmv_csr_launch(self.h, kernel, C.byref(o), d_x, d_y,
                                      stream)
        else:
            rc = _lib.spmv_csr_launch_rows(self.h, kernel, C.byref(o), d_x,
                                           d_y, rows[0], rows[1], stream)
        _check(rc, "spmv_csr_launch")

    def time(self, kernel, d_x, d_y, warmup=3, iters=20, flush_bytes=0,
             waves_per_block=0, group=0, stream=None, variant=0):
        o = _opts(waves_per_block, group, variant)
        ms = np.zeros(max(iters, 1))
        _check(_lib.spmv_csr_time(self.h, kernel, C.byref(o), d_x, d_y, warmup,
                                  iters, flush_bytes, ms.ctypes.data_as(_dp),
                                  stream), "spmv_csr_time")
        return ms[:iters]

    def download(self):
        p = _CSRp()
        _check(_lib.spmv_csr_download(self.h, C.byref(p)), "spmv_csr_download")
        return p

    def to_hll(self, col_major):
        """device conversion; the HLL handle has this handle's value type"""
        h = C.c_void_p()
        _check(_lib.spmv_hll_from_csr(self.h, int(col_major), C.byref(h)),
               "spmv_hll_from_csr")
        return HllDevice(h)


class TrsvPlan:
    """The level schedule of a sparse triangular solve, or the strict
    triangle and scratch of a sweep plan, resident in HBM (spmv_engine.h,
    spmv_trsv_plan; CsrDevice.trsv_analyse makes one)."""

    h = None
    _RANK = 1

    def __init__(self, handle):
        self.h = handle
        self.gen = _lib.spmv_handle_generation(self.h)
        if not self.gen:
            raise OSError(9, "spmv_handle_generation: %r is not a live plan "
                             "of this library" % (self.h,))
        _live.add(self)

    def _released(self):
        return not self.h

    def _release_now(self):
        self.release()

    @property
    def info(self):
        """dict(M, levels, entries, widest_level, zero_diag, launches,
        bytes)"""
        M, lv, wd, ln = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        en, zd, by = C.c_int64(), C.c_int64(), C.c_int64()
        _check(_lib.spmv_trsv_info(self.h, C.byref(M), C.byref(lv),
                                   C.byref(en), C.byref(wd), C.byref(zd),
                                   C.byref(ln), C.byref(by)),
               "spmv_trsv_info")
        return dict(M=M.value, levels=lv.value, entries=en.value,
                    widest_level=wd.value, zero_diag=zd.value,
                    launches=ln.value, bytes=by.value)

    def _sweeps(self):
        s, k = C.c_int(), C.c_int()
        _check(_lib.spmv_trsv_sweeps(self.h, C.byref(s), C.byref(k)),
               "spmv_trsv_sweeps")
        return s.value, k.value

    @property
    def sweeps(self):
        """Jacobi sweeps of one solve of a sweep plan; 0 for an exact plan"""
        return self._sweeps()[0]

    @property
    def kmax(self):
        """the most right-hand sides a solve of a sweep plan takes; 0 for an
        exact plan (which takes 1..8)"""
        return self._sweeps()[1]

    def download(self):
        """dict(level, order, level_ptr, rowptr, ja: int32; as (the stored
        values widened), diag: float64)"""
        i = self.info
        M, nz = i["M"], i["entries"]
        out = dict(level=np.zeros(M, np.int32), order=np.zeros(M, np.int32),
                   level_ptr=np.zeros(i["levels"] + 1, np.int32),
                   rowptr=np.zeros(M + 1, np.int32),
                   ja=np.zeros(nz, np.int32), diag=np.zeros(M, np.float64))
        out["as"] = np.zeros(nz, np.float64)
        _check(_lib.spmv_trsv_download(
            self.h, *(out[n].ctypes.data_as(_ip) for n in
                      ("level", "order", "level_ptr", "rowptr", "ja")),
            out["as"].ctypes.data_as(_dp), out["diag"].ctypes.data_as(_dp)),
            "spmv_trsv_download")
        return out

    def solve(self, d_B, d_X, k=1, scale=None, ldb=0, ldx=0,
              waves_per_block=0, stream=None):
        """X = T^-1 B for k = 1..8 interleaved right-hand sides (ldb, ldx >= k
        or 0), asynchronous on `stream`; d_X may be d_B (in place, ldx == ldb).
        scale: device pointer to M doubles, row i of B is multiplied by
        scale[i] first.  The bits of X are fixed by the contract in
        spmv_engine.h and depend on neither waves_per_block nor k"""
        k, ldb, ldx = int(k), int(ldb), int(ldx)
        if not 1 <= k <= 8:
            raise ValueError("k=%r: 1..8 right-hand sides per solve" % (k,))
        if (ldb and ldb < k) or (ldx and ldx < k):
            raise ValueError("ldb=%d, ldx=%d: at least k=%d (or 0)"
                             % (ldb, ldx, k))
        o = _opts(waves_per_block)
        _check(_lib.spmv_trsv_solve(self.h, C.byref(o), k, d_B, ldb, d_X, ldx,
                                    scale, stream), "spmv_trsv_solve")

    def release(self):
        h, self.h = self.h, None
        if h and _closed is False and _lib is not None:
            _lib.spmv_trsv_release_checked(h, self.gen)

    def __del__(self):
        if _closed is False:  # None / True at or after interpreter shutdown
            self.release()


class Colouring:
    """The result of CsrDevice.colour(): `colour` and `perm` (DevBuffer, M
    int32 each: the colour of every row, and new_of_old -- the new number of
    every row once the rows are ordered colour by colour), `colours`,
    `rounds`, `widest`, `narrowest` (spmv_engine.h, spmv_colour_info) and `M`.
    permute() and permute_vectors() take it where they take a permutation."""

    colour = perm = None
    _RANK = 1

    def __init__(self, A, seed, max_rounds):
        self.M = A.M
        info = ColourInfo()
        try:
            self.colour = DevBuffer(max(A.M, 1) * 4)
            self.perm = DevBuffer(max(A.M, 1) * 4)
            _check(_lib.spmv_csr_colour(A.h, seed, max_rounds,
                                        self.colour.ptr, self.perm.ptr,
                                        C.byref(info)), "spmv_csr_colour")
        except BaseException:
            self.release()
            raise
        self.colours, self.rounds = info.colours, info.rounds
        self.widest, self.narrowest = info.widest, info.narrowest
        _live.add(self)

    def _released(self):
        return self.perm is None

    def _release_now(self):
        self.release()

    def release(self):
        for buf in (self.colour, self.perm):
            if buf is not None:
                buf.free()
        self.colour = self.perm = None


class Aggregation:
    """The result of CsrDevice.aggregate(): `agg` (DevBuffer, M int32: the
    aggregate of every row), `aggregates`, `roots`, `rounds`, `widest`,
    `singletons` (spmv_engine.h, spmv_aggregate_info) and `M`."""

    agg = None
    _RANK = 1

    def __init__(self, A, theta, seed, max_rounds):
        self.M = A.M
        info = AggregateInfo()
        try:
            self.agg = DevBuffer(max(A.M, 1) * 4)
            _check(_lib.spmv_csr_aggregate(A.h, theta, seed, max_rounds,
                                           self.agg.ptr, C.byref(info)),
                   "spmv_csr_aggregate")
        except BaseException:
            self.release()
            raise
        self.aggregates, self.roots = info.aggregates, info.roots
        self.rounds, self.widest = info.rounds, info.widest
        self.singletons = info.singletons
        _live.add(self)

    def _released(self):
        return self.agg is None

    def _release_now(self):
        self.release()

    def release(self):
        if self.agg is not None:
            self.agg.free()
        self.agg = None


AmgLevel = collections.namedtuple("AmgLevel", "A P PT w")


class AmgHierarchy:
    """A smoothed-aggregation hierarchy resident in HBM (spmv_engine.h,
    spmv_amg; CsrDevice.amg makes one).  It owns its coarse operators,
    transfers, weights and scratch and borrows the fine handle (`fine`)."""

    h = None
    _RANK = 2  # released before the handle it borrows

    def __init__(self, handle, fine):
        self.h = handle
        self.fine = fine
        self.gen = _lib.spmv_handle_generation(self.h)
        if not self.gen:
            raise OSError(9, "spmv_handle_generation: %r is not a live "
                             "hierarchy of this library" % (self.h,))
        self.kmax = self._summary().kmax
        _live.add(self)

    def _released(self):
        return not self.h

    def _release_now(self):
        self.release()

    def _summary(self):
        s = AmgSummary()
        _check(_lib.spmv_amg_info(self.h, C.byref(s)), "spmv_amg_info")
        return s

    @property
    def info(self):
        """dict(levels, sweeps, coarse_sweeps, kmax, launches, complexity,
        scratch_bytes; rows, entries, rho, omega, rounds, aggregates: one
        per level)"""
        s = self._summary()
        n = s.levels
        out = dict(levels=n, sweeps=s.sweeps, coarse_sweeps=s.coarse_sweeps,
                   kmax=s.kmax, launches=s.launches, complexity=s.complexity,
                   scratch_bytes=s.scratch_bytes)
        for name in ("rows", "entries", "rho", "omega", "rounds",
                     "aggregates"):
            out[name] = list(getattr(s, name))[:n]
        return out

    def level(self, l):
        """AmgLevel(A, P, PT, w) of level l downloaded to the host: each
        matrix as (M, N, IRP, JA, AS) numpy arrays (P and PT None on the
        coarsest level), w as M doubles"""
        A, P, PT, w = (C.c_void_p() for _ in range(4))
        _check(_lib.spmv_amg_level(self.h, int(l), C.byref(A), C.byref(P),
                                   C.byref(PT), C.byref(w)),
               "spmv_amg_level")

        def host(h):
            if not h.value:
                return None
            p = _CSRp()
            _check(_lib.spmv_csr_download(h, C.byref(p)), "spmv_csr_download")
            M, N = p.contents.M, p.contents.N
            IRP, JA, AS = (np.array(a) for a in csr_arrays(p))
            csr_free(p)
            return M, N, IRP, JA, AS
        mats = [host(h) for h in (A, P, PT)]
        M = mats[0][0]
        wv = np.empty(M, np.float64)
        if M:
            _check(_lib.spmv_copy_d2h(wv.ctypes.data, w, wv.nbytes),
                   "spmv_copy_d2h")
        return AmgLevel(mats[0], mats[1], mats[2], wv)

    def apply(self, d_R, d_Z, k=1, ldr=0, ldz=0, waves_per_block=0,
              stream=None):
        """Z = V(R): one V cycle for k <= kmax interleaved vectors (ldr, ldz
        >= k or 0), asynchronous on `stream` and capturable.  The bits are
        fixed by the contract in spmv_engine.h and depend on neither
        waves_per_block nor k.  Two applies of one hierarchy must not
        overlap in time"""
        k, ldr, ldz = int(k), int(ldr), int(ldz)
        if not 1 <= k <= self.kmax:
            raise ValueError("k=%r: 1..kmax=%d vectors per apply"
                             % (k, self.kmax))
        if (ldr and ldr < k) or (ldz and ldz < k):
            raise ValueError("ldr=%d, ldz=%d: at least k=%d (or 0)"
                             % (ldr, ldz, k))
        o = _opts(waves_per_block)
        _check(_lib.spmv_amg_apply(self.h, C.byref(o), k, d_R, ldr, d_Z, ldz,
                                   stream), "spmv_amg_apply")

    def release(self):
        h, self.h = self.h, None
        if h and _closed is False and _lib is not None:
            _lib.spmv_amg_release_checked(h, self.gen)

    def __del__(self):
        if _closed is False:  # None / True at or after interpreter shutdown
            self.release()


def amg_set_fused(mode):
    """MEASUREMENT and tests: how every hierarchy sweeps from now on -- 0 by
    the composition (launch_axpby and a vector kernel), 2 by the fused kernel
    wherever it can run, 1 (the default) by the measured rule (fused from
    k = 4 on); the bits of a cycle are the same.  -> the previous mode"""
    return _check(_lib.spmv_amg_set_fused(int(mode)), "spmv_amg_set_fused")


def amg_last_phases():
    """host-clock ms of the last successful CsrDevice.amg() of this process:
    dict(rho_w, aggregate, prolongator, transpose, galerkin, finish)"""
    ms = (C.c_double * 6)()
    _lib.spmv_amg_last_phases(ms)
    return dict(zip(("rho_w", "aggregate", "prolongator", "transpose",
                     "galerkin", "finish"), ms))


def _perm_ptr(p, what):
    """the device pointer of a permutation argument: a Colouring (its .perm),
    a DevBuffer, a raw pointer, or None"""
    if isinstance(p, Colouring):
        p = p.perm
        if p is None:
            raise ValueError("%s: a released Colouring" % what)
    if isinstance(p, DevBuffer):
        if not p.ptr:
            raise ValueError("%s: a freed DevBuffer" % what)
        return p.ptr
    if p is None or isinstance(p, int):
        return p
    raise ValueError("%s=%r: a DevBuffer, a device pointer, a Colouring or "
                     "None" % (what, p))


def permute_vectors(perm, d_in, d_out, M, k=1, inverse=False, ldin=0, ldout=0,
                    stream=None):
    """k = 1..8 interleaved vectors between two numberings of the rows
    (spmv_permute_vectors): out[perm[r], j] = in[r, j], or with inverse=True
    out[r, j] = in[perm[r], j]; the bits are moved.  perm: M int32 on the
    device (a DevBuffer, a pointer or a Colouring); it is trusted.  d_in,
    d_out: device pointers or DevBuffers, not the same one.  Asynchronous on
    `stream`"""
    M, k, ldin, ldout = int(M), int(k), int(ldin), int(ldout)
    if not 1 <= k <= 8:
        raise ValueError("k=%r: 1..8 vectors per call" % (k,))
    if M < 0:
        raise ValueError("M=%d: 0 or more rows" % M)
    if (ldin and ldin < k) or (ldout and ldout < k):
        raise ValueError("ldin=%d, ldout=%d: at least k=%d (or 0)"
                         % (ldin, ldout, k))
    p = _perm_ptr(perm, "perm")
    if isinstance(d_in, DevBuffer):
        d_in = d_in.ptr
    if isinstance(d_out, DevBuffer):
        d_out = d_out.ptr
    if not p or not d_in or not d_out:
        raise ValueError("perm, d_in and d_out: device pointers, not None")
    if d_in == d_out:
        raise ValueError("d_in is d_out: the permutation is not in place")
    _check(_lib.spmv_permute_vectors(p, M, k, int(bool(inverse)), d_in, ldin,
                                     d_out, ldout, stream),
           "spmv_permute_vectors")


class SgsPreconditioner:
    """Symmetric Gauss-Seidel z = (D+U)^-1 D (D+L)^-1 r of a CsrDevice as
    pcg_trsv() takes it: `lower` and `upper` (TrsvPlan), `diag` (DevBuffer, M
    doubles); `args` = (lower, upper, diag.ptr).  CsrDevice.sgs() makes one;
    the matrix may be released afterwards."""

    lower = upper = diag = None

    def __init__(self, A, max_levels=0, sweeps=0, kmax=8):
        try:
            self.lower = A.trsv_analyse("lower", max_levels=max_levels,
                                        sweeps=sweeps, kmax=kmax)
            self.upper = A.trsv_analyse("upper", max_levels=max_levels,
                                        sweeps=sweeps, kmax=kmax)
            self.diag = DevBuffer(max(A.M, 1) * 8)
            A.diag(self.diag.ptr)
            stream_sync()
        except BaseException:
            self.release()
            raise

    @property
    def args(self):
        return self.lower, self.upper, self.diag.ptr

    def release(self):
        for plan in (self.lower, self.upper):
            if plan is not None:
                plan.release()
        if self.diag is not None:
            self.diag.free()
        self.lower = self.upper = self.diag = None


class HllDevice(_Device):
    """An HLL matrix resident in HBM (spmv_engine.h, spmv_hll_dev)."""

    _FMT = "hll"
    _NUM_KERNELS = NUM_HLL_KERNELS_ALL

    def _read_shape(self):
        M, N, NZ = C.c_int(), C.c_int(), C.c_int64()
        nb, S, cm = C.c_int(), C.c_int64(), C.c_int()
        _check(_lib.spmv_hll_shape(self.h, C.byref(M), C.byref(N),
                                   C.byref(NZ), C.byref(nb), C.byref(S),
                                   C.byref(cm)), "spmv_hll_shape")
        self.M, self.N, self.NZ = M.value, N.value, NZ.value
        self.num_blocks, self.slots = nb.value, S.value
        self.col_major = bool(cm.value)

    @classmethod
    def upload(cls, H, col_major, values="f64"):
        name = _upload_fn("hll", values)
        h = C.c_void_p()
        _check(getattr(_lib, name)(H, int(col_major), C.byref(h)), name)
        return cls(h)

    def to_index16(self):
        """a new "compact" handle with this one's pattern and values, the
        columns stored as one base per hack block + 16-bit offsets (10 / 6
        instead of 12 / 8 bytes per slot); this handle stays valid.  Column-
        major handles without wide hack blocks only; OSError(ERANGE) when the
        columns of some block span more than 65 536.  Kernels 1 and 2 give
        the bits of launch(1) on this handle"""
        h = C.c_void_p()
        self._call("to_index16", C.byref(h))
        return HllDevice(h)

    @property
    def index_bytes(self):
        """4 (int32 columns) or 2 (compact: base + 16-bit offsets)"""
        return self._call("index_bytes")

    def download_index16(self):
        """-> (base int32[num_blocks], off16 uint16[slots]) of a compact
        handle, as stored"""
        base = np.zeros(max(self.num_blocks, 1), np.int32)
        off16 = np.zeros(max(self.slots, 1), np.uint16)
        self._call("download_index16", base.ctypes.data_as(_ip),
                   off16.ctypes.data_as(C.POINTER(C.c_uint16)))
        return base[:self.num_blocks], off16[:self.slots]

    def kernel_bytes(self, kernel):
        """bytes one launch of `kernel` must move: 12 per STORED slot (8 with
        fp32 values; 10 / 6 on a compact handle) for the direct kernels, 12
        per true entry for the blocked copy (no padding)"""
        return _lib.spmv_hll_kernel_bytes(self.h, kernel)

    def launch(self, kernel, d_x, d_y, waves_per_block=0, stream=None,
               blocks=None, variant=0):
        o = _opts(waves_per_block, 0, variant)
        if blocks is None:
            rc = _lib.spmv_hll_launch(self.h, kernel, C.byref(o), d_x, d_y,
                                      stream)
        else:
            rc = _lib.spmv_hll_launch_blocks(self.h, kernel, C.byref(o), d_x,
                                             d_y, blocks[0], blocks[1], stream)
        _check(rc, "spmv_hll_launch")

    def time(self, kernel, d_x, d_y, warmup=3, iters=20, flush_bytes=0,
             waves_per_block=0, stream=None, variant=0, group=0):
        o = _opts(waves_per_block, group, variant)
        ms = np.zeros(max(iters, 1))
        _check(_lib.spmv_hll_time(self.h, kernel, C.byref(o), d_x, d_y, warmup,
                                  iters, flush_bytes, ms.ctypes.data_as(_dp),
                                  stream), "spmv_hll_time")
        return ms[:iters]


# ---------------------------------------------------------------- vectors
_sig("vec_create", Vec, C.c_size_t)
_sig("vec_fill", None, C.POINTER(Vec), C.c_double)
_sig("vec_fill_random", None, C.POINTER(Vec))
_sig("vec_fill_synth", None, C.POINTER(Vec), C.c_uint64, C.c_int64)


def vec_random(n, reseed=True):
    """The reference's x: rand()/RAND_MAX in index order.  reseed=True puts
    the C library generator in its never-seeded state first (srand(1))."""
    if reseed:
        _libc.srand(1)
    v = _lib.vec_create(n)
    _lib.vec_fill_random(C.byref(v))
    return _take_vec(v)


def vec_synth(n, seed=7, first=0):
    v = _lib.vec_create(n)
    _lib.vec_fill_synth(C.byref(v), seed, first)
    return _take_vec(v)


def compute_gflops(ms, nnz):
    """2*nnz / (ms*1e6), 0 for ms <= 0 (reference utils.h:70-75)."""
    return (2.0 * nnz) / (ms * 1e6) if ms > 0.0 else 0.0


# ---------------------------------------------------------------- multi-GPU (C)
_sig("spmv_mgpu_create", C.c_int, C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_mgpu_create_rehearsal", C.c_int, C.c_int, C.POINTER(C.c_void_p))
_sig("spmv_mgpu_destroy", None, C.c_void_p)
_sig("spmv_mgpu_load_csr", C.c_int, C.c_void_p, _CSRp, C.c_int)
_sig("spmv_mgpu_generate", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
     C.c_int64, C.c_uint64, C.c_int)
_sig("spmv_mgpu_load_csr_part", C.c_int, C.c_void_p, _CSRp, C.c_int, C.c_int)
_sig("spmv_mgpu_generate_part", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int,
     C.c_int64, C.c_uint64, C.c_int, C.c_int)
_sig("spmv_mgpu_set_ragged_exchange", C.c_int, C.c_void_p, C.c_int)
_sig("spmv_mgpu_set_logical_shards", C.c_int, C.c_void_p, C.c_int, C.c_int)
_sig("spmv_mgpu_set_exchange_engine", C.c_int, C.c_void_p, C.c_int)
_sig("spmv_mgpu_partition", C.c_int, C.c_void_p, _ip, C.POINTER(C.c_int64))
_sig("spmv_mgpu_build_panels", C.c_int, C.c_void_p, C.POINTER(PanelOpts))
_sig("spmv_mgpu_set_x", C.c_int, C.c_void_p, _dp)
_sig("spmv_mgpu_fill_x", C.c_int, C.c_void_p, C.c_uint64)
_sig("spmv_mgpu_spmv", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp)
_sig("spmv_mgpu_autotune", C.c_int, C.c_void_p, _ip)
_sig("spmv_mgpu_run", C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, _dp, _dp)
_sig("spmv_mgpu_exchange_only", C.c_int, C.c_void_p, C.c_int, _dp)
_sig("spmv_mgpu_set_exchange", C.c_int, C.c_void_p, C.c_int, C.c_int)
_sig("spmv_mgpu_rccl_version", C.c_int)
_sig("spmv_mgpu_comm_ranks", C.c_int, C.c_void_p)
_sig("spmv_mgpu_device_bus_id", C.c_int, C.c_void_p, C.c_int, C.c_char_p,
     C.c_size_t)
_sig("spmv_mgpu_shard_info", C.c_int, C.c_void_p, C.c_int,
     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_size_t)
_sig("spmv_device_pci_bus_id", C.c_int, C.c_int, C.c_char_p, C.c_size_t)
_sig("spmv_mgpu_get_y", C.c_int, C.c_void_p, C.c_int, _dp)
_sig("spmv_mgpu_info", C.c_int, C.c_void_p, _ip, _ip, C.POINTER(C.c_int64),
     C.POINTER(C.c_int64))


class MultiGpu:
    """Single-process multi-GPU SpMV (spmv_mgpu.h): row shards + RCCL
    all-gather of y, as the C driver's `-g N` runs it."""

    h = None
    _RANK = 2

    def __init__(self, ngpus, rehearsal=False):
        """rehearsal: `ngpus` LOGICAL devices on the visible card(s), no RCCL
        communicator, copies instead of collectives (spmv_mgpu.h)"""
        h = C.c_void_p()
        if rehearsal:
            _check(_lib.spmv_mgpu_create_rehearsal(ngpus, C.byref(h)),
                   "spmv_mgpu_create_rehearsal")
        else:
            _check(_lib.spmv_mgpu_create(ngpus, C.byref(h)),
                   "spmv_mgpu_create")
        self.h, self.n = h, ngpus
        _live.add(self)

    def _released(self):
        return not self.h

    def _release_now(self):
        self.destroy()

    PARTITIONS = {"even": 0, "nnz": 1}
    RAGGED_EXCHANGES = {"p2p": 0, "bcast": 1, "padded": 2}

    def load_csr(self, A, as_hll=False, partition="even"):
        """partition "nnz": near-equal entries per device (ragged fragments)"""
        _check(_lib.spmv_mgpu_load_csr_part(
            self.h, A, int(as_hll), self.PARTITIONS[partition]),
            "spmv_mgpu_load_csr_part")
        self.M = A.contents.M

    def generate(self, kind, rows_per_gpu, K, W, seed=42, as_hll=True,
                 partition="even"):
        _check(_lib.spmv_mgpu_generate_part(
            self.h, kind, rows_per_gpu, K, W, seed, int(as_hll),
            self.PARTITIONS[partition]), "spmv_mgpu_generate_part")
        self.M = rows_per_gpu * self.n

    ENGINES = {"rccl": 0, "copy": 1}

    def set_exchange_engine(self, engine="rccl"):
        """"rccl": collectives (default); "copy": peer copies on the copy
        engines (no kernel competes with the SpMV for CUs)"""
        _check(_lib.spmv_mgpu_set_exchange_engine(self.h, self.ENGINES[engine]),
               "spmv_mgpu_set_exchange_engine")

    def set_logical_shards(self, shards=1, reserve_cus=0):
        """from the next load / generate on: every device's rows as `shards`
        matrices (the blocked path then overlaps shard c's all-gather with
        shard c+1's kernel); reserve_cus: CUs a sweep copy leaves to RCCL"""
        _check(_lib.spmv_mgpu_set_logical_shards(self.h, shards, reserve_cus),
               "spmv_mgpu_set_logical_shards")

    def set_ragged_exchange(self, kind="p2p"):
        """how ragged fragments travel: p2p | bcast | padded"""
        _check(_lib.spmv_mgpu_set_ragged_exchange(
            self.h, self.RAGGED_EXCHANGES[kind]),
            "spmv_mgpu_set_ragged_exchange")

    def partition(self):
        """-> (starts[n+1], entries[n], ragged?)"""
        st = (C.c_int * (self.n + 1))()
        ent = (C.c_int64 * self.n)()
        rg = _check(_lib.spmv_mgpu_partition(self.h, st, ent),
                    "spmv_mgpu_partition")
        return list(st), list(ent), bool(rg)

    def set_x(self, x):
        x, xp = _as_d(x)
        _check(_lib.spmv_mgpu_set_x(self.h, xp), "spmv_mgpu_set_x")

    def fill_x(self, seed=7):
        _check(_lib.spmv_mgpu_fill_x(self.h, seed), "spmv_mgpu_fill_x")

    def build_panels(self, sched=None, tile_rows=0, deterministic=None):
        """the blocked copy on every shard (needed before running the blocked
        kernel id without autotune())"""
        o = _panel_opts(0, sched, tile_rows, deterministic=deterministic)
        _check(_lib.spmv_mgpu_build_panels(self.h, C.byref(o)),
               "spmv_mgpu_build_panels")

    def autotune(self):
        """-> kernel id measured fastest for the loaded shards"""
        k = C.c_int()
        _check(_lib.spmv_mgpu_autotune(self.h, C.byref(k)),
               "spmv_mgpu_autotune")
        return k.value

    def spmv(self, kernel=-1, warmup=1, iters=3):
        ms = np.zeros(max(iters, 1))
        _check(_lib.spmv_mgpu_spmv(self.h, kernel, warmup, iters,
                                   ms.ctypes.data_as(_dp)), "spmv_mgpu_spmv")
        return ms[:iters]

    def run(self, kernel, warmup, steps):
        """the bench shape (spmv_mgpu_run): -> (wall ms of the `steps` steps,
        per-device mean kernel ms)"""
        wall = C.c_double()
        kms = np.zeros(self.n)
        _check(_lib.spmv_mgpu_run(self.h, kernel, warmup, steps,
                                  C.byref(wall), kms.ctypes.data_as(_dp)),
               "spmv_mgpu_run")
        return wall.value, kms

    def set_exchange(self, chunks=1, force=False):
        """chunks > 1: staged all-gathers overlapped with the next chunk's
        kernel (direct kernels); force: run the collective with one device"""
        _check(_lib.spmv_mgpu_set_exchange(self.h, chunks, int(force)),
               "spmv_mgpu_set_exchange")

    def exchange_only(self, iters=10):
        ms = C.c_double()
        _check(_lib.spmv_mgpu_exchange_only(self.h, iters, C.byref(ms)),
               "spmv_mgpu_exchange_only")
        return ms.value

    def comm_ranks(self):
        return _lib.spmv_mgpu_comm_ranks(self.h)

    def bus_ids(self):
        out = []
        for r in range(self.n):
            buf = C.create_string_buffer(32)
            _check(_lib.spmv_mgpu_device_bus_id(self.h, r, buf, 32),
                   "spmv_mgpu_device_bus_id")
            out.append(buf.value.decode())
        return out

    def shard_info(self, rank=0):
        """-> (stored slots / entries, algorithmic bytes, blocked layout or "")"""
        st, by = C.c_int64(), C.c_int64()
        buf = C.create_string_buffer(256)
        _check(_lib.spmv_mgpu_shard_info(self.h, rank, C.byref(st),
                                         C.byref(by), buf, 256),
               "spmv_mgpu_shard_info")
        return st.value, by.value, buf.value.decode()

    def info(self):
        """-> (ngpus, rows per gpu, nnz total, algorithmic bytes per gpu)"""
        n, r = C.c_int(), C.c_int()
        nz, by = C.c_int64(), C.c_int64()
        _check(_lib.spmv_mgpu_info(self.h, C.byref(n), C.byref(r),
                                   C.byref(nz), C.byref(by)), "spmv_mgpu_info")
        return n.value, r.value, nz.value, by.value

    def get_y(self, rank=0):
        y = np.zeros(self.M)
        _check(_lib.spmv_mgpu_get_y(self.h, rank, y.ctypes.data_as(_dp)),
               "spmv_mgpu_get_y")
        return y

    def destroy(self):
        h, self.h = self.h, None
        if h and _closed is False and _lib is not None:
            _lib.spmv_mgpu_destroy(h)

    def __del__(self):
        if _closed is False:  # None / True at or after interpreter shutdown
            self.destroy()


# experiment knob of the harness (tools/README.md): the library reads no
# environment, so its process default schedule is set from here
if os.environ.get("SPMV_PANEL_SCHED") in PANEL_SCHED:
    _lib.spmv_set_panel_schedule(PANEL_SCHED[os.environ["SPMV_PANEL_SCHED"]])
