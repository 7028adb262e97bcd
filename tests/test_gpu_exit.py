"""Process exit with device objects still alive, and the dead-handle contract.

A failed test's traceback keeps the test's locals -- an autotuned HllDevice
carrying a blocked copy, two DevBuffers -- alive until the interpreter exits.
Each case below is a CHILD process that ends in exactly such a state without
releasing anything; it must exit 0 and print nothing that smells of heap
corruption.  The child runs with tools/abort_trace.c preloaded, so a native
abort would name its stack in the assertion message.

History: these cases were written in round 3 against the `double free or
corruption` abort of round 2's GPU test process, whose cause was then
unknown.  Round 4 found it -- the binding loaded the library RTLD_GLOBAL and a
later in-process `import torch` collided with its dependency closure
(tests/test_rocm_runtime_once.py reproduces that without a GPU) -- so what
this file guards is the lifetime rule itself: an atexit hook releases live
objects in dependency order while the HIP runtime is up, finalisers are no-ops
afterwards, every entry point answers -EBADF for a dead handle, and a release
the library ignores is counted (spmv_ignored_releases)."""
import os
import subprocess
import sys

import pytest

import spmv_scpa_amd as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import faulthandler, sys
faulthandler.enable()
sys.path.insert(0, %(root)r)
import spmv_scpa_amd as S

def build():
    # columns anywhere: the selector leaves the direct kernels for the
    # blocked path (tune_blocked swaps keep / cand / original copies)
    M, N = 2_000_000, 16_000_000
    dA = S.CsrDevice.generate(S.SYNTH_RANDOM, M, N, 32, 1 << 30, 0, 42)
    dH = dA.to_hll(True)
    dA.release()
    d_x, d_y = S.DevBuffer(N * 8), S.DevBuffer(M * 8)
    S.dev_fill_synth(d_x.ptr, N, 7)
    best, ms = dH.autotune(d_x.ptr, d_y.ptr)
    assert best == S.HLL_KERNEL_PANELS, best
    dH.launch(best, d_x.ptr, d_y.ptr)
    S.stream_sync()
    return dH, d_x, d_y

mode = sys.argv[1]
kept = []
if mode == "globals":          # module globals, torn down at finalisation
    dH, d_x, d_y = build()
elif mode == "traceback":      # what pytest keeps of a failed test
    def failing_test():
        dH, d_x, d_y = build()
        like = S.CsrDevice.generate(S.SYNTH_BANDED, 100_000, 100_000, 16, 0, 0, 42)
        raise AssertionError("the test fails before release()")
    try:
        failing_test()
    except AssertionError:
        kept.append(sys.exc_info())
elif mode == "cycle":          # garbage only the cycle collector can free
    class Box:
        pass
    b = Box()
    b.me, b.objs = b, build()
    del b
elif mode == "double":         # explicit release, then finalisers again
    dH, d_x, d_y = build()
    h = dH.h
    dH.release()
    assert S.ignored_releases() == 0
    S._lib.spmv_hll_release(h)         # ignored by the library, and counted
    assert S.ignored_releases() == 1
    assert S._lib.spmv_live_handles() == 0
    dH2 = S.HllDevice.__new__(S.HllDevice)
    dH2.h, dH2.gen = h, 1              # a second wrapper of a dead handle
    assert S._lib.spmv_hll_launch(h, 1, None, d_x.ptr, d_y.ptr, None) == -9
elif mode == "mgpu":           # communicator + shards left alive
    g = S.MultiGpu(1)
    g.generate(S.SYNTH_RANDOM, 64_000, 32, 4096)
    g.fill_x()
    g.spmv(-1, 1, 2)
print("child-ok", mode, len(S.live_objects()), S._lib.spmv_live_handles())
"""

BAD = ("double free", "corruption", "core dumped", "Aborted", "abort_trace",
       "Segmentation", "Fatal Python error", "free():", "munmap_chunk",
       "malloc():")


@pytest.mark.parametrize("mode", ["globals", "traceback", "cycle", "double",
                                  "mgpu"])
def test_exit_with_live_device_objects_is_clean(mode, tmp_path):
    script = tmp_path / "child.py"
    script.write_text(CHILD % {"root": ROOT})
    env = dict(os.environ)
    pre = os.path.join(ROOT, "spmv_scpa_amd", "bin", "libabort_trace.so")
    if os.path.exists(pre):
        env["LD_PRELOAD"] = pre
    r = subprocess.run([sys.executable, str(script), mode],
                       capture_output=True, text=True, timeout=600, env=env)
    tail = (r.stdout + "\n---- stderr ----\n" + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "child-ok " + mode in r.stdout, tail
    for word in BAD:
        assert word not in r.stderr, tail


def test_release_is_idempotent_and_counted():
    """in-process: a handle released explicitly is gone from the library's
    live set; a second release (raw) changes nothing and is COUNTED; every
    entry point answers -EBADF for the dead handle before touching it"""
    import ctypes as C
    before = S._lib.spmv_live_handles()
    ign = S.ignored_releases()
    dA = S.CsrDevice.generate(S.SYNTH_BANDED, 50_000, 50_000, 16, 0, 0, 42)
    dH = dA.to_hll(True)
    assert S._lib.spmv_live_handles() == before + 2
    assert 0 < dA.gen < dH.gen  # generations only grow
    raw = dH.h
    dH.release()
    dH.release()            # the wrapper forgot the handle: not a library call
    assert S.ignored_releases() == ign
    S._lib.spmv_hll_release(raw)
    assert S.ignored_releases() == ign + 1
    assert S._lib.spmv_live_handles() == before + 1
    EBADF = -9
    buf = C.create_string_buffer(64)
    k, ms = C.c_int(), C.c_double()
    o = S._panel_opts()
    for rc in (S._lib.spmv_hll_shape(raw, None, None, None, None, None, None),
               S._lib.spmv_hll_algorithmic_bytes(raw),
               S._lib.spmv_hll_kernel_bytes(raw, 4),
               S._lib.spmv_hll_build_panels(raw, 0),
               S._lib.spmv_hll_build_panels_opts(raw, C.byref(o)),
               S._lib.spmv_hll_build_panels_as(raw, 0, 2, 0),
               S._lib.spmv_hll_build_panels_like(raw, raw),
               S._lib.spmv_hll_panels_info(raw, None, None, None, None),
               S._lib.spmv_hll_panels_schedule(raw),
               S._lib.spmv_hll_panels_layout(raw, C.byref(o), None),
               S._lib.spmv_hll_panels_set_waves(raw, 4),
               S._lib.spmv_hll_panels_tile_rows(raw),
               S._lib.spmv_hll_panels_describe(raw, buf, 64),
               S._lib.spmv_hll_release_source(raw),
               S._lib.spmv_hll_tune_log(raw, buf, 64),
               S._lib.spmv_hll_time(raw, 1, None, None, None, 0, 1, 1 << 30,
                                    C.byref(ms), None),
               S._lib.spmv_hll_autotune(raw, None, None, 1, C.byref(k),
                                        C.byref(ms))):
        assert rc == EBADF, rc
    assert S._lib.spmv_handle_generation(raw) == 0
    dA.release()
    assert S._lib.spmv_live_handles() == before
    assert dA not in S.live_objects() and dH not in S.live_objects()


def test_release_checked_acts_only_on_its_own_generation():
    """a LIVE handle released with a generation that is not its own (what a
    stale wrapper would present after the allocator reused the address):
    ignored, counted, the handle stays alive"""
    d = S.CsrDevice.generate(S.SYNTH_BANDED, 4_096, 4_096, 4, 0, 0, 42)
    addr, gen = d.h.value, d.gen
    ign = S.ignored_releases()
    S._lib.spmv_csr_release_checked(addr, gen + 1000)
    assert S.ignored_releases() == ign + 1
    S._lib.spmv_csr_release_checked(addr, 0)       # 0 never matches: refused
    assert S._lib.spmv_handle_generation(addr) == gen   # still alive
    d_x, d_y = S.DevBuffer(4_096 * 8), S.DevBuffer(4_096 * 8)
    d.launch(2, d_x.ptr, d_y.ptr)
    S.stream_sync()
    d.release()
    assert S._lib.spmv_handle_generation(addr) == 0


def test_stale_wrapper_cannot_release_a_newer_handle_at_the_same_address():
    """the allocator may hand a released handle's address out again: the
    checked release acts only on the generation the wrapper was created with.
    Whether ONE freed address comes back depends on what else the process has
    allocated and freed in that size class (the runtime's own objects, every
    test collected before this one), so 32 handles are released and a new
    handle on ANY of their addresses will do (skipped when none of 64 lands on
    one; the test above covers the same check without relying on the
    allocator)"""
    def new_handle():
        return S.CsrDevice.generate(S.SYNTH_BANDED, 4_096, 4_096, 4, 0, 0, 42)

    firsts = [new_handle() for _ in range(32)]
    stale = {d.h.value: d.gen for d in firsts}  # address -> dead generation
    for d in firsts:
        d.release()
    # create handles until one lands on an old address (calloc of one size
    # class: usually the very next one)
    made, twin = [], None
    for _ in range(64):
        d = new_handle()
        made.append(d)
        if d.h.value in stale:
            twin = d
            break
    try:
        if twin is None:
            pytest.skip("the allocator did not reuse any of the addresses")
        addr, gen = twin.h.value, stale[twin.h.value]
        assert twin.gen != gen
        ign = S.ignored_releases()
        S._lib.spmv_csr_release_checked(addr, gen)   # the stale wrapper
        assert S.ignored_releases() == ign + 1
        d_x, d_y = S.DevBuffer(4_096 * 8), S.DevBuffer(4_096 * 8)
        twin.launch(2, d_x.ptr, d_y.ptr)             # still alive
        S.stream_sync()
    finally:
        for d in made:
            d.release()


def test_waves_per_block_zero_restores_the_size_based_default():
    S._lib.set_csr_waves_per_block(2)
    S._lib.set_csr_waves_per_block(0)   # back to auto (was: clamped to 1)
    S._lib.set_hll_waves_per_block(0)
    dA = S.CsrDevice.generate(S.SYNTH_BANDED, 50_000, 50_000, 16, 0, 0, 42)
    d_x, d_y = S.DevBuffer(50_000 * 8), S.DevBuffer(50_000 * 8)
    dA.launch(2, d_x.ptr, d_y.ptr)
    S.stream_sync()
    dA.release()
