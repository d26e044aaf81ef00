"""The field primitives one at a time (tests/prim): every primitive of gl.h, gl_dev.h, gl_limb.h, fp252.h and the accumulators of
eval_kernels.h against Python big-integer arithmetic, on inputs drawn per edge class (one class per carry, wrap or borrow fix-up).

emu: the simulator build (the headers' host branches) against the reference, in the CPU suite.
hip: the device build (hipcc, gfx950: inline assembly, builtins, constant-address-space loads) against the reference, and word for
word against the simulator build on the same inputs -- weak values, raw limbs and raw accumulator columns included.  The device
runs in one child process of its own, under a time limit."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "prim"))
import prims  # noqa: E402

CPU_N = 6           # inputs per drawn class in the CPU suite
GPU_N = {"gl": 2048, "gld": 256, "limb": 256, "acc": 512, "f252": 1024}      # ... on the device: 2^14.5 .. 2^15.6 cases per family
GPU_N["rpo"] = 64   # the reference of this family costs 1.6 ms per permutation: 170 states in all forms, 2^10 inputs per S-box class


def _report(ops_):
    for o in ops_:
        print("[field_prims]", o.summary())
        assert o.counts and all(c > 0 for c in o.counts.values()), o.summary()


@pytest.fixture(scope="module")
def host_lib():
    return prims.Lib(prims.build("host"))


@pytest.mark.parametrize("family", prims.FAMILIES)
def test_emu(family, host_lib):
    ops_ = prims.ops(family, CPU_N)
    _report(ops_)
    bad = []
    for o in ops_:
        bad += o.verify(host_lib.run(o))
    assert not bad, "\n".join(bad[:20])


@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    ops_ = {f: prims.ops(f, GPU_N[f]) for f in prims.FAMILIES}
    flat = [o for f in prims.FAMILIES for o in ops_[f]]
    so = prims.build("device")
    d = tmp_path_factory.mktemp("field_prims")
    inp, outp = str(d / "in.npz"), str(d / "out.npz")
    prims.save_inputs(inp, flat)
    r = subprocess.run([sys.executable, os.path.join(prims.HERE, "prims.py"), "device", so, inp, outp],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "device run failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = np.load(outp)
    return ops_, {id(o): res["out%d" % j] for j, o in enumerate(flat)}


@pytest.mark.gpu
@pytest.mark.parametrize("family", prims.FAMILIES)
def test_hip_reference(family, device_run):
    ops_, outs = device_run
    _report(ops_[family])
    bad = []
    for o in ops_[family]:
        bad += o.verify(outs[id(o)])
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("family", prims.FAMILIES)
def test_hip_matches_host(family, device_run, host_lib):
    ops_, outs = device_run
    bad = []
    for o in ops_[family]:
        host, dev = host_lib.run(o), outs[id(o)]
        if not np.array_equal(host, dev):
            i = int(np.flatnonzero((host != dev).any(axis=1))[0])
            bad.append("%s [%s] case %d in=%s: device %s host %s" % (o.key, o.label[i], i, prims._hx(o.rows[i]),
                                                                    prims._hx(dev[i].tolist()), prims._hx(host[i].tolist())))
    assert not bad, "\n".join(bad[:20])
