"""GroupNorm + LeakyReLU backward, without a GPU: the float64 specification of normbwdutil agrees with float64 autograd, the
inputs the GPU tests use keep S1 and S2 away from zero and the gate band's exclusions under the cap, a float32 restatement of
the kernels' arithmetic lies inside the derived bounds in three summation orders, and every deliberate defect (normbwdutil.MUTANTS)
violates them on every case it applies to - so a kernel with such a defect cannot pass test_gpu_norm_bwd.py."""
from __future__ import annotations

import numpy as np
import pytest

import normbwdutil as NB

DTS = [NB.BF16, NB.F16, NB.F32]
_CASES = {}


def cases(dt):
    if dt not in _CASES:
        _CASES[dt] = NB.all_cases(dt)
    return _CASES[dt]


def test_spec_matches_float64_autograd():
    """Once, on inputs without ties or kinks: every consumer kind, channel window, pad offset and blend weight."""
    dt = NB.F32
    A = (2, 32, 18, 26)
    todo = [NB.make_case("pad+pool", dt, A, ["pad", "pool"], 1), NB.make_case("pool_odd", dt, (2, 32, 19, 27), ["plain", "pool"], 2),
            NB.make_case("up", dt, A, ["up"], 3), NB.make_case("same2", dt, (1, 16, 6, 40), ["plain", "plain0"], 4),
            NB.make_case("head", dt, (1, 16, 33, 7), ["head"], 5),
            NB.make_case("blend1", dt, A, ["plain0"], 6, alpha=0.3, wm=1), NB.make_case("blend2", dt, A, ["plain0"], 7, alpha=1.5, wm=2)]
    for k in todo:
        ref, auto = NB.spec(k), NB.autograd_reference(k)
        assert not ref["excluded"].any()
        for name, want in auto.items():
            err = float(np.abs(ref[name] - want).max() / np.abs(want).max())
            print(f"{k.name} {name}: {err:.2e}")
            assert err <= 1e-9, (k.name, name, err)


@pytest.mark.parametrize("dt", DTS, ids=[NB.DTNAME[d] for d in DTS])
def test_inputs_have_power_and_exclusions_stay_under_the_cap(dt):
    for k in cases(dt):
        ref = NB.spec(k, k.stats32(), stores_g=k.stores_g, shuffled=k.shuffled)
        frac = float(ref["excluded"].mean())
        s1, s2 = np.abs(ref["S1"]).min(), np.abs(ref["S2"]).min()
        print(f"{k.name}: left out {frac:.2e}, min |S1| {s1:.3f}, min |S2| {s2:.3f}")
        assert frac <= NB.CAP, (k.name, frac)
        assert s1 >= 0.1 and s2 >= 0.1, (k.name, s1, s2)
        if k.ties or k.kink:
            assert not ref["excluded"].any(), k.name           # exact ties and exact zeros only: nothing is left to chance
        if k.ties and k.pooled:          # most windows tie, at every pair of positions, three- and four-way too
            n, c, h, w = k.shape
            live = np.broadcast_to((k.gamma != 0).reshape(1, c, 1, 1, 1), (n, c, h // 2, w // 2, 4))
            pre = k.x * (k.gamma.reshape(1, c, 1, 1))
            aw = NB.windows(np.where(pre > 0, pre, 0.2 * pre))
            eq = (aw == aw.max(-1, keepdims=True)) & live
            cnt = eq.sum(-1)
            assert (cnt[live[..., 0]] >= 2).mean() > 0.5 and (cnt == 3).any() and (cnt == 4).any()
            for i in range(4):
                for j in range(i + 1, 4):
                    assert (eq[..., i] & eq[..., j]).any(), (k.name, i, j)
            pool = [q for q in k.cons if q.kind == "pool"][0]
            assert np.abs(pool.da).min() >= 0.5
            scale = np.abs(k.gamma)[None, :] * np.repeat(k.stats32()[1], c // NB.G, axis=1)
            assert ((scale == 0) | (scale >= 0.25)).all()
        if k.kink:
            mean, rstd = k.stats32()
            pre = k.x * (k.gamma.reshape(1, c_of(k), 1, 1) * np.repeat(rstd, c_of(k) // NB.G, axis=1)[:, :, None, None])
            assert 0.25 < float((pre == 0).mean()) < 0.45 and (mean == 0).all()


def c_of(k):
    return k.shape[1]


@pytest.mark.parametrize("dt", DTS, ids=[NB.DTNAME[d] for d in DTS])
def test_restatement_is_inside_the_bounds_and_every_mutant_is_outside(dt):
    survivors, outside = [], []
    for k in cases(dt):
        ref = NB.spec(k, k.stats32(), stores_g=k.stores_g, shuffled=k.shuffled)
        worst = {}
        for order in range(3):
            rng = np.random.default_rng(1000 + order)
            good = NB.ratios(NB.restate(k, rng, None, k.stores_g), ref)
            for name, v in good.items():
                worst[name] = max(worst.get(name, 0.0), v)
            if max(good.values()) > 1.0:
                outside.append((k.name, order, good))
            for m in NB.MUTANTS:
                if not NB.mutant_applies(m, k):
                    continue
                r = NB.ratios(NB.restate(k, np.random.default_rng(1000 + order), m, k.stores_g), ref)
                hit = r["dgamma"] if m == "dgamma_gx" else r["dx"]
                if not hit > 1.0:
                    survivors.append((k.name, m, order, hit))
        print(f"{NB.DTNAME[dt]} {k.name}: restatement / bound " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))
    assert not outside, outside
    assert not survivors, survivors


@pytest.mark.parametrize("dt", DTS, ids=[NB.DTNAME[d] for d in DTS])
def test_routing_sets_tell_the_first_maximum_from_the_others(dt):
    """The exact check of which elements take the pooled gradient (normbwdutil.routing_sets, used by the GPU tests on the pooled
    ties and kink cases): the restatement's set equals the specification's, a wrong tie rule or a pool taken on x gives another,
    and at least three quarters of the elements can be told apart."""
    for k in cases(dt):
        if not (k.pooled and (k.ties or k.kink)):
            continue
        ref = NB.spec(k, k.stats32(), stores_g=k.stores_g, shuffled=k.shuffled)
        for m in (None, "tie_last", "tie_all", "pool_on_x"):
            if m and not NB.mutant_applies(m, k):
                continue
            out = NB.restate(k, np.random.default_rng(7), m, k.stores_g)
            if not k.stores_g:
                del out["g"]
            got, want, live = NB.routing_sets(out, ref)
            assert live.mean() >= 0.75, (k.name, live.mean())
            assert np.array_equal(got, want) == (m is None), (k.name, m, int((got != want).sum()))
