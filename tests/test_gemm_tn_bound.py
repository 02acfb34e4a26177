"""Keeps tests/gemm_tn_ref.py honest without a GPU, at every (shape, K, k_splits, layout) test_gpu_gemm_tn_elementwise.py runs
(one list, gemm_tn_ref.CASES) and for both K-tile sizes of csrc/gemm_tn.hip (32: ring and wide kernels, 64: two-buffer kernel):

* the bound admits a right implementation with room: `emulate` <= 0.25 of it on `real`, and equals the fp64 reference bit for bit
  on `exact`;
* the bound refuses every wrong turn of `mutate`: > 2.0 of it on `real` and bit-unequal on `exact`, at every combination where the
  turn changes anything;
* where a turn changes nothing is stated by gemm_tn_ref.is_noop from the mutation's definition, and the observed set is exactly
  that set on both families; no mutation is a no-op everywhere, and all but one are live in more than half of the combinations
  (`stale_stage` needs a split of five K-tiles, which is what it is about).

0.25 and 2.0 are conditions on the bound, not measurements.  -s prints the model's worst ratio and every mutation's smallest."""
import pytest
import torch

import gemm_tn_ref as T

K_TILES = [32, 64]


@pytest.fixture(scope="module")
def sweep():
    """every combination once: {(k_tile, Mo, No, K, S, lay): (model ratio, exact equal, {mutation: (ratio or None, exact unequal
    or None)})}, None where the mutation left the model's output bit-identical"""
    res = {}
    for Mo, No in T.SHAPES:
        for K, S, lay in T.CASES:
            ops = {}
            for fam in T.FAMILIES:
                _, xv, _, _, yv, _ = T.operands(fam, Mo, No, K, lay, finite_fill=True)
                want, absacc = T.reference(xv[:K], yv[:K])
                ops[fam] = (xv, yv, want, T.bound(absacc, K, S))
            for kt in K_TILES:
                xr, yr, wr, br = ops["real"]
                xe, ye, we, _ = ops["exact"]
                base_r, base_e = T.emulate(xr, yr, K, S, kt), T.emulate(xe, ye, K, S, kt)
                muts = {}
                for name in T.MUTATIONS:
                    mr, me = T.mutate(name, xr, yr, K, S, kt), T.mutate(name, xe, ye, K, S, kt)
                    muts[name] = (None if torch.equal(mr, base_r) else T.worst_ratio(mr, wr, br),
                                  None if torch.equal(me, base_e) else not torch.equal(me, we.float()))
                res[(kt, Mo, No, K, S, lay)] = (T.worst_ratio(base_r, wr, br), torch.equal(base_e, we.float()), muts)
    return res


def test_cases_cover_what_the_kernels_branch_on():
    """the list itself: K-tile counts 1..7 and 10 (ring, wide) and 1..5 (two-buffer), every K with every layout, every split count
    with every layout, an empty trailing split, a split of one tile, and the integer family's range"""
    assert sorted({-(-K // 32) for K in T.KS}) == [1, 2, 3, 4, 5, 6, 7, 10]
    assert sorted({-(-K // 64) for K in T.KS}) == [1, 2, 3, 4, 5]
    for K in T.KS:
        assert {lay for k, _, lay in T.CASES if k == K} == set(T.LAYOUTS)
    for S in T.SPLITS:
        assert {lay for _, s, lay in T.CASES if s == S} == set(T.LAYOUTS)
    assert len(T.CASES) == len(T.KS) * len(T.SPLITS)
    tiles = [T.split_tiles(K, S, 32) for K, S, _ in T.CASES]
    assert any(not t[-1] for t in tiles) and any(len(t) > 1 and len(t[1]) == 1 for t in tiles)
    assert any(len(t[0]) != len(t[-1]) and t[-1] for t in tiles)          # an uneven tail
    for seed in (31, 32, 33, 34):
        p = T.pool("exact", seed).float()
        assert float(p.abs().min()) == 1 and float(p.abs().max()) == 4 and torch.equal(p, p.round())
        assert {float(v) for v in p.unique()} == {-4.0, -3.0, -2.0, -1.0, 1.0, 2.0, 3.0, 4.0}
    assert 16 * max(T.KS) < 2 ** 14


def test_split_tiles_is_the_kernels_partition():
    """gemm_tn.hip: per = ceil(nkt / S); kbase = split * per; nkt_split = clamp(nkt - kbase, 0, per)"""
    for K in T.KS:
        for S in T.SPLITS:
            for kt in K_TILES:
                nkt = (K + kt - 1) // kt
                per = (nkt + S - 1) // S if S > 1 else nkt
                got = T.split_tiles(K, S, kt)
                assert len(got) == S
                for s, ts in enumerate(got):
                    n = max(0, min(per, nkt - s * per))
                    assert ts == list(range(s * per, s * per + n))
                assert sorted(t for ts in got for t in ts) == list(range(nkt))


def test_the_bound_admits_the_model(sweep):
    worst = {kt: max(v[0] for k, v in sweep.items() if k[0] == kt) for kt in K_TILES}
    print(f"gemm_tn model / bound, worst over {len(sweep)} combinations: " + ", ".join(f"k_tile {k}: {w:.4f}" for k, w in worst.items()))
    bad = [(k, v[0]) for k, v in sweep.items() if not v[0] <= 0.25]
    assert not bad, bad[:5]
    assert all(v[1] for v in sweep.values()), [k for k, v in sweep.items() if not v[1]][:5]


@pytest.mark.parametrize("name", T.MUTATIONS)
def test_the_bound_refuses_the_mutation(sweep, name):
    live, noop = {}, []
    for key, (_, _, muts) in sweep.items():
        kt, Mo, No, K, S, lay = key
        ratio, unequal = muts[name]
        expect_noop = T.is_noop(name, Mo, No, K, S, lay, kt)
        assert (ratio is None) == expect_noop and (unequal is None) == expect_noop, (name, key, ratio, unequal)
        if expect_noop:
            noop.append(key)
        else:
            live[key] = ratio
            assert ratio > 2.0 and unequal, (name, key, ratio, unequal)
    for kt in K_TILES:
        n_live = sum(1 for k in live if k[0] == kt)
        n_all = sum(1 for k in sweep if k[0] == kt)
        assert n_live > 0, (name, kt)
        if name != "stale_stage":
            assert 2 * n_live > n_all, (name, kt, n_live, n_all)
    print(f"{name}: live at {len(live)} of {len(sweep)} combinations, smallest ratio {min(live.values()):.1f}, largest "
          f"{max(live.values()):.3g}; no-op at {len(noop)} (gemm_tn_ref.is_noop)")
