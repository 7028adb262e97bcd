"""Root cause of the `double free or corruption (!prev)` abort at the exit of
round 2's GPU test process (gpurun_out/r2c4_1.log) and of round 4's first run
with an in-process `import torch` (gpurun_out/r4c2_1.log) -- reproduced and
pinned WITHOUT a GPU: the children below only import.

The binding loaded libspmv_scpa_amd.so with RTLD_GLOBAL; the symbols of its
dependency closure (librccl -> librocm_smi64) became process-global, a later
`import torch` bound against them, and glibc aborted inside exit().  The
binding now loads with RTLD_LOCAL and keeps ONE copy of the ROCm runtime in
the process, whatever the import order.

Round 6: WHICH copy.  The library is built by
/opt/rocm's hipcc; torch's wheel bundles an older HIP.  A process that does
not need torch -- the tests, `python bench.py` at one GPU -- binds the
system runtime the library was built for (hip_built == hip_runtime) and
refuses a later `import torch`; a process that imported torch first (the
ranks of an N > 1 run) shares torch's copy and says `mismatch`."""
import importlib.util
import os
import signal
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import os, re, sys
sys.path.insert(0, %(root)r)
%(imports)s
seen = {}
for line in open("/proc/self/maps"):
    m = re.search(r"(/\S+\.so\S*)$", line.strip())
    if m:
        base = re.sub(r"\.so.*", ".so", os.path.basename(m.group(1)))
        seen.setdefault(base, set()).add(os.path.realpath(m.group(1)))
for lib in ("libamdhip64.so", "librccl.so", "libhsa-runtime64.so"):
    print("COPIES", lib, len(seen.get(lib, ())), sorted(seen.get(lib, ())))
print("child-ok")
"""

# the two wordings glibc's free() has used for the abort of the RTLD_GLOBAL
# child, same build, same image: the first as root in a working tree, the
# second as an ordinary user in a clean checkout
GLIBC_FREE_ABORTS = ("double free or corruption", "free(): invalid pointer")

needs_torch = pytest.mark.skipif(importlib.util.find_spec("torch") is None,
                                 reason="torch is not installed")


def run_child(imports, **env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c",
                        CHILD % {"root": ROOT, "imports": imports}],
                       capture_output=True, text=True, timeout=600, env=env)
    copies = {l.split()[1]: int(l.split()[2])
              for l in r.stdout.splitlines() if l.startswith("COPIES")}
    return r, copies


REPORT = ("import json; print('REPORT', json.dumps("
          "spmv_scpa_amd.rocm_runtime_report()))")


def report_of(r):
    import json
    line = [l for l in r.stdout.splitlines() if l.startswith("REPORT")][-1]
    return json.loads(line.split(" ", 1)[1])


@needs_torch
@pytest.mark.parametrize("imports,env,bound", [
    # the order that aborted in round 2: now refused, loudly, by the guard
    ("import spmv_scpa_amd\n"
     "try:\n    import torch\n    print('TORCH imported')\n"
     "except ImportError as e:\n    print('TORCH refused:', e)\n" + REPORT,
     {}, "system"),
    # ... unless the process says up front that torch is coming
    ("import spmv_scpa_amd\nimport torch\n" + REPORT,
     {"SPMV_ROCM_RUNTIME": "torch"}, "torch"),
    # bench.py's ranks, the dist workers: torch first
    ("import torch\nimport spmv_scpa_amd\n" + REPORT, {}, "torch"),
    # never imports torch: tests, tools, `python bench.py` at one GPU
    ("import spmv_scpa_amd\n" + REPORT, {}, "system"),
], ids=["ours_then_torch_refused", "ours_then_torch_announced",
        "torch_then_ours", "ours_only"])
def test_one_rocm_runtime_whatever_the_import_order(imports, env, bound):
    r, copies = run_child(imports, **env)
    tail = r.stdout[-1500:] + "\n---- stderr ----\n" + r.stderr[-1500:]
    assert r.returncode == 0, tail
    assert "child-ok" in r.stdout, tail
    for word in ("double free", "corruption", "Aborted", "core dumped"):
        assert word not in r.stderr, tail
    assert copies["libamdhip64.so"] == 1 and copies["librccl.so"] == 1, tail
    assert copies["libhsa-runtime64.so"] <= 1, tail
    rep = report_of(r)
    assert rep["bound"] == bound and rep["runtimes_mapped"] == 1, rep
    if "refused" in (imports + " ") and bound == "system" and "try:" in imports:
        assert "TORCH refused:" in r.stdout and "import torch BEFORE".lower() \
            in r.stdout.lower(), tail
    if bound == "system":
        # VERDICT r05 next #5, "done": the runtime the code was built for
        assert rep["hip_from"].startswith("/opt/rocm"), rep
        assert rep["hip_built"].split(".")[:2] == \
            rep["hip_runtime"].split(".")[:2], rep
        assert rep["mismatch"] is False and not rep["shared_with_torch"]
    else:
        assert rep["hip_from"] == "torch/lib" and rep["shared_with_torch"]
        # flagged exactly when torch's bundled HIP is another major.minor
        assert rep["mismatch"] == (rep["hip_built"].split(".")[:2] !=
                                   rep["hip_runtime"].split(".")[:2]), rep


def test_the_single_gpu_bench_path_never_imports_torch():
    """`python bench.py` at one GPU takes device memory, stream and events
    from the library's C-ABI (benchlib.devshim): its process binds the system
    runtime, so the driver's line carries hip_built == hip_runtime.  Checked
    here without a GPU: building the job object imports what the run imports
    (it then stops at 'no GPU visible')."""
    code = ("import sys\nsys.path.insert(0, %r)\n"
            "import bench\nfrom benchlib import dist\n"
            "args = bench.parse_args([])\n"
            "try:\n    dist.RankJob(args, 1)\n"
            "except SystemExit as e:\n    print('EXIT', e)\n"
            "print('TORCH' if 'torch' in sys.modules else 'NO-TORCH')\n"
            "import spmv_scpa_amd as S\nprint('BOUND', S.ROCM_RUNTIME_BOUND)\n"
            % ROOT)
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "NO-TORCH" in r.stdout and "BOUND system" in r.stdout, r.stdout


@needs_torch
def test_the_abort_was_the_global_load_and_nothing_else():
    """the old way of loading, restated with bare ctypes: the library with
    RTLD_GLOBAL, then torch -- an abort at exit on a box without a GPU, with
    no handle ever created.  (Documents the cause; skipped should a future
    torch / ROCm pairing no longer collide.)"""
    lib = os.path.join(ROOT, "spmv_scpa_amd", "lib", "libspmv_scpa_amd.so")
    code = ("import ctypes\n"
            "ctypes.CDLL(%r, mode=ctypes.RTLD_GLOBAL)\n"
            "import torch\nprint('imports done')\n" % lib)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, timeout=600)
    assert "imports done" in r.stdout
    if r.returncode == 0:
        pytest.skip("RTLD_GLOBAL + torch no longer collide on this image")
    # glibc aborts at the first of its heap checks that the mixed-up free()
    # meets; which one depends on the layout of the heap (the library's
    # load-time allocations, its path, the environment), not on the cause
    assert r.returncode == -signal.SIGABRT, (r.returncode, r.stderr[-500:])
    assert any(said in r.stderr for said in GLIBC_FREE_ABORTS), r.stderr[-500:]
    # ... and the same two loads with RTLD_LOCAL leave cleanly
    r = subprocess.run([sys.executable, "-c",
                        code.replace("RTLD_GLOBAL", "RTLD_LOCAL")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "double free" not in r.stderr, r.stderr


def test_elf_reader_and_runtime_report():
    """the binding's ELF reader names what the loader will match on, and the
    import-time check sees one runtime copy of each library"""
    sys.path.insert(0, ROOT)
    import spmv_scpa_amd as S
    soname, needed = S._elf_dynamic(S.LIB_PATH)
    assert any(n.startswith("libamdhip64.so.") for n in needed), needed
    assert any(n.startswith("librccl.so.") for n in needed), needed
    assert S._elf_dynamic(__file__) == (None, [])
    assert S.ROCM_RUNTIME_ONCE is True
    assert all(len(v) == 1 for v in S.mapped_rocm_runtimes().values())
    if S.ROCM_RUNTIME_SHARED_WITH_TORCH:
        for path in S.ROCM_RUNTIME_SHARED_WITH_TORCH:
            name = os.path.basename(path)
            assert S._elf_dynamic(path)[0] in [
                n for n in needed if n.startswith(name)], path


@needs_torch
def test_a_bundled_runtime_with_another_soname_is_not_preloaded(tmp_path):
    """a torch wheel whose libamdhip64 carries another SONAME
    (another ROCm major) must not be preloaded -- the loader would not take it
    for the library's DT_NEEDED name and two runtimes would be mapped.  Staged
    with a fake `torch` package whose lib/ holds a copy of /opt/rocm's HIP
    runtime patched to SONAME libamdhip64.so.6."""
    src = "/opt/rocm/lib/libamdhip64.so"
    if not os.path.exists(src):
        pytest.skip("no /opt/rocm runtime to stage the fake wheel from")
    pkg = tmp_path / "torch"
    (pkg / "lib").mkdir(parents=True)
    (pkg / "__init__.py").write_text("raise ImportError('fake torch')\n")
    data = open(os.path.realpath(src), "rb").read()
    assert data.count(b"libamdhip64.so.7\0") >= 1
    (pkg / "lib" / "libamdhip64.so").write_bytes(
        data.replace(b"libamdhip64.so.7\0", b"libamdhip64.so.6\0"))
    code = ("import sys, warnings\n"
            "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "with warnings.catch_warnings(record=True) as w:\n"
            "    warnings.simplefilter('always')\n"
            "    import spmv_scpa_amd as S\n"
            "print('SHARED', S.ROCM_RUNTIME_SHARED_WITH_TORCH)\n"
            "print('WARNED', [str(x.message)[:60] for x in w])\n"
            "print('MAPS', S.mapped_rocm_runtimes())\n" % (ROOT, str(tmp_path)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, timeout=300,
                       env=dict(os.environ, SPMV_ROCM_RUNTIME="torch"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SHARED None" in r.stdout, r.stdout
    assert "SONAME" in r.stdout and "libamdhip64.so.6" not in r.stdout.split(
        "MAPS")[1], r.stdout


@needs_torch
def test_a_build_check_may_import_torch_afterwards():
    """__graft_entry__.build() imports the package to check its symbols and
    does no device work: it lifts the guard (spmv_scpa_amd.allow_torch_import)
    so that whoever called it can still import torch in that process"""
    code = ("import sys\nsys.path.insert(0, %r)\n"
            "import spmv_scpa_amd as S\n"
            "assert S.ROCM_TORCH_IMPORT_GUARDED and S.ROCM_RUNTIME_BOUND == 'system'\n"
            "S.allow_torch_import()\nimport torch\nprint('TORCH', torch.__version__)\n"
            % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and "TORCH " in r.stdout, r.stderr[-2000:]
    for word in ("double free", "corruption", "Aborted", "core dumped"):
        assert word not in r.stderr, r.stderr[-2000:]
