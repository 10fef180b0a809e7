"""CPU (-m "not gpu"): the population acting entries (include/gcrl.h gcrl_pop_observe_act, gcrl_pop_process_step,
gcrl_pop_acting_counts) refuse a null handle, null arrays and a bad mode with the field named and before any device work — so they do
so on a machine without a GPU — and the build lints (tools/check_release_isa.py) cover the two population acting kernels: the flag
store of rowchain_act_pop_kernel follows a drained publication, and neither kernel uses per-thread scratch."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refused(gcrl, rc, field):
    msg = gcrl._ffi.last_error()
    assert rc == gcrl._ffi.GCRL_ERR_ARG and field in msg, (rc, msg)


def test_observe_act_refusals(gcrl):
    lib = gcrl._ffi.lib
    x = (C.c_float * 64)()
    out = (C.c_double * 64)()
    modes = (C.c_int32 * 1)(1)
    call = lambda pop, obs, dg, md, o: lib.gcrl_pop_observe_act(pop, None, None, obs, 7, dg, 3, 2, None, md, o, None)
    _refused(gcrl, call(None, None, x, modes, out), "obs_host")
    _refused(gcrl, call(None, x, None, modes, out), "dg_host")
    _refused(gcrl, call(None, x, x, None, out), "modes")
    _refused(gcrl, call(None, x, x, modes, None), "out_host")
    for bad in (-2, 3, 7):
        modes[0] = bad
        _refused(gcrl, call(None, x, x, modes, out), "modes")
    modes[0] = -1
    _refused(gcrl, call(None, x, x, modes, out), "pop")
    modes[0] = 2
    _refused(gcrl, call(None, x, x, modes, out), "pop")


def test_process_step_refusals(gcrl):
    lib = gcrl._ffi.lib
    x = (C.c_float * 64)()
    dn = (C.c_uint8 * 8)()
    rings = (C.c_void_p * 1)()
    rows = (C.c_int64 * 1)()

    def call(pop=None, rings=rings, obs=x, dg=x, act=x, rows=rows):
        return lib.gcrl_pop_process_step(pop, rings, None, 1, None, 0, obs, x, 7, dg, x, None, x, act, x, dn, 0, 2, rows, None)
    _refused(gcrl, call(rings=None), "rings")
    _refused(gcrl, call(obs=None), "obs_host")
    _refused(gcrl, call(dg=None), "dg_host")
    _refused(gcrl, call(act=None), "actions_host")
    _refused(gcrl, call(rows=None), "rows_out")
    _refused(gcrl, call(), "pop")


def test_acting_counts_refuses_null_handle(gcrl):
    v = [C.c_int64(-5) for _ in range(5)]
    _refused(gcrl, gcrl._ffi.lib.gcrl_pop_acting_counts(None, *[C.byref(a) for a in v]), "pop")
    assert all(a.value == -5 for a in v)


def test_population_classes_have_the_acting_surface(gcrl):
    for cls in (gcrl.DDPGPopulation, gcrl.TD3Population):
        for name in ("observe_act", "process_step", "acting_counts"):
            assert callable(getattr(cls, name)), (cls.__name__, name)


def test_isa_lints_cover_the_population_acting_kernels():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_release_isa.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "release check: PASS" in r.stdout and "scratch check: PASS" in r.stdout
    lines = r.stdout.splitlines()
    assert any("rowchain_act_pop_kernel" in l and "flag store after s_waitcnt vmcnt(0): ok" in l for l in lines), r.stdout[-3000:]
    for kernel in ("rowchain_act_pop_kernel", "her_process_step_pop_kernel"):
        assert any(kernel in l and "0 bytes of scratch per thread: ok" in l for l in lines), kernel
