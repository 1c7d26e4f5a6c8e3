"""CPU: the C-ABI calls of the conv autograd host path (tpgan_ops conv2d / conv2d_group / linear /
conv2d_folded, both tuners, the double-backward Functions) against the recorded ledger
tests/golden/conv_calls.json -- see tests/golden/make_conv_calls.py for the stub library, the
scenarios and the layout.  The fixture was generated on the commit before the per-launch
descriptors; it is not regenerated from a tree that means to keep the calls as they are."""
import importlib.util
import json
import os

import pytest
import torch

import tpgan_lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_conv_calls", os.path.join(GOLDEN, "make_conv_calls.py"))
M = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(M)


@pytest.fixture(scope="module")
def recorded():
    with open(M.OUT) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fresh():
    return M.generate()


def test_scenario_list(recorded):
    assert list(recorded["scenarios"]) == [name for name, _ in M.SCENARIOS]
    assert os.path.getsize(M.OUT) < os.path.getsize(os.path.join(GOLDEN, "wgrad_plans.json"))


@pytest.mark.parametrize("name", [name for name, _ in M.SCENARIOS])
def test_calls_match_the_record(recorded, fresh, name):
    want, got = M.expand(recorded, name), M.expand(fresh[0], name)
    for i, (a, b) in enumerate(zip(want, got)):
        if a != b:
            diff = ["  arg %d: recorded %r\n          now      %r" % (j, p, q)
                    for j, (p, q) in enumerate(zip(a, b)) if p != q]
            if a[0] == b[0] and any(isinstance(p, dict) for p in a):
                da, db = [next(p for p in r if isinstance(p, dict)) for r in (a, b)]
                diff += ["  desc.%s: recorded %r, now %r" % (k, da[k], db.get(k)) for k in da if da[k] != db.get(k)]
            pytest.fail("%s: call %d differs\n recorded %s\n now      %s\n%s" % (
                name, i, json.dumps(a), json.dumps(b), "\n".join(diff)), pytrace=False)
    assert len(want) == len(got), "%s: %d calls recorded, %d now; first extra: %s" % (
        name, len(want), len(got), json.dumps((want + got)[min(len(want), len(got))]))


def test_ledger_is_deterministic(fresh):
    again, _ = M.generate()
    assert again == fresh[0]


def test_unread_descriptor_fields_are_zero(fresh):
    """Every descriptor handed to the library carries only what that entry point reads: no plan
    pick of another launch (data_ksplit in a tpg_conv2d_bwd_filter call), no left-over in_act."""
    bad = []
    for name, raw in fresh[1].items():
        for k, (fn, full) in enumerate(raw):
            extra = {f: v for f, v in full.items() if f not in M.READS.get(fn, M.BASE) and v != 0}
            if extra:
                bad.append("%s: descriptor call %d (%s) carries %s" % (name, k, fn, extra))
    assert not bad, "\n".join(bad[:20])


def _retained(E, fail):
    """conv2d with a link_dx and a parked gradient; backward with `fail` answering, then again on
    the retained graph with nothing parked and nothing failing.  -> descriptors of the second."""
    ops = E.ops
    link = ops.GradLink()
    x = E.act("x", 2, 8, 6, 6, M.BF16)
    w, b = E.weight("w", 8, 8, 3)
    with ops.compute_dtype(M.BF16):
        y = ops.conv2d(x, w, b, pad=M.P1, act=M.LEAKY, link_dx=link)
    gy = E.act("gy", 2, 8, 6, 6, M.BF16, grad=False)
    link.g = ops.new_act(2, 8, 6, 6, M.BF16, "cpu")
    E.rec.fail = fail
    with pytest.raises(RuntimeError):
        y.backward(gy, retain_graph=True)
    E.rec.fail = None
    link.g = None
    del E.rec.raw[:]
    y.backward(gy, retain_graph=True)
    return list(E.rec.raw)


def test_failed_launch_leaves_no_state():
    once = []

    def fail(fn, d):
        if fn == "tpg_conv2d_bwd" and not once:
            once.append(d)
            return -1
        return 0
    out = []
    M.run_scenario(lambda E: out.extend(_retained(E, fail)))
    assert once and once[0]["flags"] & L.FLAG_DX_ACCUM  # (the failed launch was the accumulating one)
    bwd = [d for fn, d in out if fn == "tpg_conv2d_bwd"]
    assert len(bwd) == 1
    assert bwd[0]["flags"] & L.FLAG_DX_ACCUM == 0
    assert bwd[0]["act"] == L.ACT_LEAKY and bwd[0]["in_act"] == 0


def test_failed_wgrad_sweep_leaves_no_state():
    """A launch of the weight-gradient sweep fails (not with the -30 of an uncovered tile): the
    next backward of the node carries no algo / ksplit of the aborted sweep."""
    def fail(fn, d):
        return -1 if fn == "tpg_conv2d_bwd_filter" and (d["algo"], d["ksplit"]) == (2, 2) else 0
    out = []

    def scenario(E):
        E.ops.AUTOTUNE["enabled"] = True
        out.extend(_retained(E, fail))
    M.run_scenario(scenario)
    bwd = [d for fn, d in out if fn == "tpg_conv2d_bwd"]
    assert len(bwd) == 1 and (bwd[0]["algo"], bwd[0]["ksplit"]) == (0, 0), bwd
    sweep = [(d["algo"], d["ksplit"]) for fn, d in out if fn == "tpg_conv2d_bwd_filter"]
    assert sweep[0] == (1, 1) and (2, 2) in sweep  # (the sweep starts over, and now gets past the pick that failed)
