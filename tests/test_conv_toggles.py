"""The conv-engine kernels behind process-wide switches of libdro_amd.so.

DRO_K7_FWD (fwd_k7s2_kernel), DRO_K7_WGRAD_OFF (the 7x7 weight gradients on
wgrad_kernel) and DRO_CONV_NO_THIN (the thin 7x7 shapes on igemm_kernel) are
each read once into
a static, so the suite's own process never takes the other branch.  Each
switch gets one fresh child process (python -m tests.conv_variants --subset
NAME) that runs the table cases the switch re-routes with the same fp64
checks as tests/test_conv_variants.py and asserts that the switched kernels
are in the launch log and the default ones are not.  The children run one
after another; a child that dies on a signal or runs into its time limit
ends the sequence (nothing more is started on the device after a fault).
"""
import os
import subprocess
import sys

import pytest

import conv_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 240          # seconds per child: import + a handful of small cases
ORDER = ["k7fwd", "k7wgradoff", "nothin"]
_RESULTS = {}


def _run_children():
    """All children, in order, once per session; stops at the first child that
    was killed by a signal or by its time limit."""
    if _RESULTS:
        return _RESULTS
    stopped = None
    for subset in ORDER:
        if stopped is not None:
            _RESULTS[subset] = (None, f"not started: the {stopped} child died on a signal or its time limit")
            continue
        env = dict(os.environ)
        env[V.TOGGLES[subset][0]] = "1"
        try:
            p = subprocess.run([sys.executable, "-m", "tests.conv_variants", "--subset", subset], cwd=ROOT, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=LIMIT)
            _RESULTS[subset] = (p.returncode, p.stdout[-6000:])
            if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
                stopped = subset
        except subprocess.TimeoutExpired as e:
            out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
            _RESULTS[subset] = (None, "time limit\n" + out[-6000:])
            stopped = subset
    return _RESULTS


def test_subsets_exist():
    for subset in ORDER:
        assert any(subset in c.subsets for c in V.CASES), subset
    k7 = [c for c in V.CASES if "k7fwd" in c.subsets]
    # Cin 3 (the padded zero column) and 6, odd input sizes, Cout no multiple of 64, B = 3,
    # more output tiles than blocks (4 tiles per block: the prefetch loop repeats)
    assert {c.cin for c in k7} == {3, 6}
    assert any(c.H % 2 and c.W % 2 and c.cout % 64 and c.B == 3 for c in k7)
    for c in k7:
        ho, wo = V.out_hw(c)
        assert c.B * -(-ho // 8) * -(-wo // 8) > 4


@pytest.mark.gpu
@pytest.mark.parametrize("subset", ORDER)
def test_switched_kernels(subset):
    rc, out = _run_children()[subset]
    assert rc == 0, (subset, V.TOGGLES[subset][0], rc, out)
