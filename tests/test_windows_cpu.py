"""CPU-only checks of the coalesced publish windows: the library exports the new
entry points and refuses a NULL context, and the combining queue
(emqx_amd/csrc/gm_combine.h) passes its stand-alone ThreadSanitizer program."""

import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("emqx_gm_match_windows", "emqx_gm_combiner_open", "emqx_gm_combiner_match", "emqx_gm_combiner_stats",
       "emqx_gm_combiner_close")


def test_library_exports_the_window_calls():
    from emqx_amd import _lib
    L = _lib.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "emqx_gpu_match.h")).read()
    for name in NEW + ("emqx_gm_window", "emqx_gm_combiner_opts", "emqx_gm_combiner_stats_t"):
        assert name in hdr, name


def test_null_context_is_einval():
    from emqx_amd import _lib
    L = _lib.lib()
    w = (_lib.Window * 1)()
    m, d = (_lib.Csr * 1)(), (_lib.Csr * 1)()
    m[0].n_rows = d[0].n_rows = 77  # (no output is touched)
    assert L.emqx_gm_match_windows(None, None, w, 1, 0, m, d) == _lib.EINVAL
    assert m[0].n_rows == 77 and d[0].n_rows == 77
    h = ctypes.c_void_p(5)
    assert L.emqx_gm_combiner_open(None, None, ctypes.byref(h)) == _lib.EINVAL
    assert h.value == 5
    assert L.emqx_gm_combiner_match(None, None, None, None, 0, 0, m, d) == _lib.EINVAL
    assert L.emqx_gm_combiner_stats(None, None) == _lib.EINVAL
    assert L.emqx_gm_combiner_close(None) == _lib.EINVAL


def test_struct_layouts_match_the_header():
    """The ctypes mirrors of the new structs: sizes as the C compiler lays them out."""
    from emqx_amd import _lib
    src = ('#include "emqx_gpu_match.h"\n#include <stdio.h>\nint main(void){printf("%zu %zu %zu\\n",'
           "sizeof(emqx_gm_window),sizeof(emqx_gm_combiner_opts),sizeof(emqx_gm_combiner_stats_t));return 0;}\n")
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "s.c"), os.path.join(td, "s")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.Window), ctypes.sizeof(_lib.CombinerOpts), ctypes.sizeof(_lib.CombinerStats)]


def test_combining_queue_under_tsan():
    """tests/asan/tsan_combiner.cpp: gm_combine.h alone with a stub executor under
    ThreadSanitizer, run as a plain executable (nothing preloaded): 8 threads x
    200 calls get their own results, min_windows = 4 forms one group of four,
    incompatible windows are never mixed, groups respect max_windows and
    max_topics, an executor error reaches exactly its group, close waits."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "emqx_amd", "csrc"), "tsan-combiner"], capture_output=True,
                       text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1:exitcode=66")
    p = subprocess.run([os.path.join(ROOT, "tests", "asan", "tsan_combiner")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert p.returncode == 0, (p.stdout[-1000:], p.stderr[-3000:])
    assert "tsan_combiner ok" in p.stdout
