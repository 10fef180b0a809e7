"""CPU (-m "not gpu"): the BatchNorm actors' population acting entry (include/gcrl.h gcrl_pop_observe_act_bn; csrc/agent_pop.inc) is
declared, exported and bound, and refuses a null handle and null arrays with the argument named and before any device work — so it
does so on a machine without a GPU.  The build lints (tools/check_release_isa.py) cover its two kernels (csrc/act_bn.hip): the flag
store of act_bn_pop_kernel follows a drained publication, and neither form uses per-thread scratch.  (The refusals that need a
population, hence a device: tests/test_gpu_population_sac_acting.py.)"""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refused(gcrl, rc, field):
    msg = gcrl._ffi.last_error()
    assert rc == gcrl._ffi.GCRL_ERR_ARG and "gcrl_pop_observe_act_bn" in msg and field in msg, (rc, msg)


def test_entry_is_declared_exported_and_bound(gcrl):
    header = open(os.path.join(ROOT, "include", "gcrl.h")).read()
    assert re.search(r"^int gcrl_pop_observe_act_bn\(gcrl_pop\* p,", header, re.M)
    fn = gcrl._ffi.lib.gcrl_pop_observe_act_bn          # (ctypes raises AttributeError for a symbol the library does not export)
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert callable(gcrl.SACPopulation._native_observe_act)
    assert gcrl.SACPopulation._native_observe_act is not gcrl.TD3Population._native_observe_act


def test_refusals_name_the_argument(gcrl):
    lib = gcrl._ffi.lib
    x = (C.c_float * 64)()
    eps = (C.c_double * 64)()
    out = (C.c_double * 64)(*([7.0] * 64))
    call = lambda pop, obs, dg, o, e=None: lib.gcrl_pop_observe_act_bn(pop, None, None, obs, 7, dg, 3, 2, e, o, None)
    _refused(gcrl, call(None, None, x, out), "obs_host")
    _refused(gcrl, call(None, x, None, out), "dg_host")
    _refused(gcrl, call(None, x, x, None), "out_host")
    _refused(gcrl, call(None, x, x, out), "pop")
    _refused(gcrl, call(None, x, x, out, eps), "pop")
    assert all(v == 7.0 for v in out)


def test_isa_lints_cover_the_population_forms():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_release_isa.py"), "--units", "act_bn.hip"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "release check: PASS" in r.stdout and "scratch check: PASS" in r.stdout
    lines = r.stdout.splitlines()
    assert any("act_bn_pop_kernel" in l and "flag store after s_waitcnt vmcnt(0): ok" in l for l in lines), r.stdout[-3000:]
    for kernel in ("act_bn_pop_kernel", "act_bn_pop_staged_kernel"):
        assert any(kernel in l and "0 bytes of scratch per thread: ok" in l for l in lines), kernel
