"""The line-major node stage of the fp64 far-field loop, restated in numpy (tests/node_pass_ref.py): the properties the
kernel's ff_classify_batch_np / ff_node_pass rely on, and that the regions of tests/test_gpu_node_pass.py can show the
errors such a pass can make.  No GPU."""
import numpy as np
import pytest

import node_pass_cases as nc
import node_pass_ref as npr
import tile_moments_ref as tm

# The fractions' stated accuracy for node values at the lower ends of their ranges is 4e-13 / 2e-13 / 9e-13 of the value
# (vamp_hip.hip, ff_eval2).  Measured here on the regions below, restated sums against scipy's wofz relative to the sum of
# the terms' magnitudes: worst 1.5e-13 (P4196, K = 7).  The bar is four times that.
FAR_BAR = 6e-13


def test_model_reproduces_the_design_figures():
    x, nat = npr.headline_natives(W=8)
    old, new = np.array([npr.model_costs(n, x) for n in nat]).mean(0)
    print(f"headline: tile by tile {old:.1f}, line-major {new:.1f} lane-instructions per tile")
    assert abs(old - 113.0) < 2.0 and abs(new - 104.0) < 2.0


@pytest.mark.parametrize("kind", ["up", "down", "steps"])
def test_edge_class_is_deep_enough_for_every_node(kind):
    """for random walkers: the class a line is folded into is at least the class every node of every tile of the batch
    needs for which the line is far"""
    P = 4352
    x = np.arange(P) - (P - 1) / 2.0
    if kind == "down":
        x = x[::-1].copy()
    if kind == "steps":
        x = np.cumsum(np.where((np.arange(P) // 256) % 2 == 0, 1.0, 2.0))
        x = x - 0.5 * (x[0] + x[-1])
    rng = np.random.default_rng(5)
    checked = 0
    for _ in range(40):
        K = 16
        nat = np.stack([rng.uniform(0.2, 3, K), rng.uniform(x.min() - 300, x.max() + 300, K), 10.0 ** rng.uniform(-2, 2.5, K),
                        10.0 ** rng.uniform(0.3, 2.6, K)], axis=1)
        far = tm.classify(nat[None], x)[0][0]
        need = npr.depth_of(npr.node_r2(nat, x).min(-1))            # [K, nt]
        for sets in npr.class_sets(nat, x):
            for k in range(K):
                for t in sets["tiles"]:
                    if far[k, t]:
                        assert sets["far"] >> k & 1
                        assert npr.set_depth(sets, k) >= need[k, t], (k, t)
                        checked += 1
            assert sets["n6"] & ~sets["n4"] == 0 and sets["n4"] & ~sets["n3"] == 0 and sets["n3"] & ~sets["far"] == 0
    assert checked > 1000


@pytest.mark.parametrize("K", nc.KS)
@pytest.mark.parametrize("name", list(nc.SHAPES))
def test_restated_sums_match_wofz(name, K):
    c = nc.case(name, K)
    got, mag, _ = npr.node_sums(c["t"], c["x"])
    want = npr.node_sums_exact(c["t"], c["x"])
    err = np.max(np.abs(got - want) / np.maximum(mag, 1e-300))
    print(f"{name} K={K}: restated node sums against wofz, worst {err:.2e} of the terms' magnitudes")
    assert err <= FAR_BAR


@pytest.mark.parametrize("name", list(nc.SHAPES))
def test_regions_cover_the_conditions(name):
    """K = 16: some full batch holds all four depth classes, one of them with an odd number of lines; some line is far for
    three tiles of a batch and near, or wide, for the fourth.  K = 7: a line far for three and near for the
    fourth.  K = 1: the line is far from some tiles and near to others.  (P2304 has no full batch: nothing to cover.)"""
    for K in nc.KS:
        c = nc.case(name, K)
        assert np.isfinite(c["want"]).all()
        far, wide, near = [m[0] for m in tm.classify(c["t"][None], c["x"])]
        sets = npr.class_sets(c["t"], c["x"])
        if name == "P2304":
            assert not sets and far.any() and near.any()
            continue
        assert sets
        if K == 1:
            assert far.any() and near.any()
            continue
        assert any((far[k, s["tiles"]].sum() == 3) and (near | wide)[k, s["tiles"]].any() for s in sets for k in range(K))
        if K == 16:
            ok = False
            for s in sets:
                counts = [bin(m).count("1") for m in (s["n6"], s["n4"] & ~s["n6"], s["n3"] & ~s["n4"], s["far"] & ~s["n3"])]
                ok |= all(n > 0 for n in counts) and any(n % 2 for n in counts)
            assert ok


@pytest.mark.parametrize("plant", ["rowshift", "nearfar", "widefar"])
def test_planted_errors_move_the_log_posterior(plant):
    """each error moves the log-posterior of P4096, K = 16 beyond the GPU tests' bar of 1e-9 max(1, |lnprob|)"""
    c = nc.case("P4096", 16)
    args = (c["t"], c["x"], c["flux"], c["noise"])
    good = npr.chi2_from_nodes(*args, npr.node_sums(c["t"], c["x"])[0])
    bad = npr.chi2_from_nodes(*args, npr.node_sums(c["t"], c["x"], plant=plant)[0])
    shift, bar = 0.5 * abs(bad - good), 1e-9 * max(1.0, abs(c["want"][0]))
    print(f"{plant}: log-posterior moves by {shift:.3e}, bar {bar:.3e}")
    assert shift > bar


def test_a_class_too_shallow_moves_the_node_sums():
    """Every class folded one level too shallow.  On P4096, K = 16 this moves the log-posterior by 5.3e-11 against a bar of
    3.0e-6: a fraction one level short is still good to 1e-10 .. 1e-9 of a wing's value, which no log-posterior test at
    1e-9 max(1, |lnprob|) can see on data with noise of 0.05.  The test that sees it is the comparison of the node sums
    themselves (tests/test_gpu_node_pass.py, 64 ulps of the terms' magnitudes): the error must exceed that bar."""
    c = nc.case("P4096", 16)
    good, mag, _ = npr.node_sums(c["t"], c["x"])
    bad = npr.node_sums(c["t"], c["x"], plant="shallow")[0]
    full = npr.batches(c["x"].size // 256)[0].reshape(-1)
    excess = np.max(np.abs(bad - good)[full] / (64 * 2.0 ** -53 * mag[full]))
    print(f"shallow: node sums move by up to {excess:.1f} times the bar of the GPU comparison")
    assert excess > 4.0
