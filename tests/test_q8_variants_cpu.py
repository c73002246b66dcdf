"""What tests/test_q8_variants_gpu.py covers, counted without a GPU, and its tied fractions checked on the oracle alone.

1. The named lists of q8_variants_common, mapped through variant_of / init_variant_of (the mirror of dispatch_variant and
   launch_update in csrc/mpmvs_api.hip), reach all 40 instantiations of k_update and all 24 of k_init.
2. The seeded sweep: over fuzz_common.draw(k), k < Q8_FUZZ_CASES, every update variant is launched by at least two cases, every
   init variant by at least one, and every bucket edge of the view counts is drawn in both texel formats; Q8_FUZZ_CASES is the
   smallest multiple of 50 of which that holds.
3. The tie scene: its homographies are exact translations, the three relations between its views hold in the oracle's 8-bit
   arithmetic, in the exact-fraction arithmetic the three views around every tie all differ, and the costs compared are mostly real
   costs, not the sentinel."""
import numpy as np
import pytest

import fuzz_common
import q8_variants_common as q8c
from update_variants_common import ALL_INIT_VARIANTS, ALL_UPDATE_VARIANTS, init_variant_of, run_variants, variant_of


def test_variant_of_mirrors_the_dispatch():
    assert len(ALL_UPDATE_VARIANTS) == 40 and len(ALL_INIT_VARIANTS) == 24
    assert [variant_of(V, True, "photometric", 0)[1] for V in (1, 8, 9, 16, 17, 24, 25, 32)] == [8, 8, 16, 16, 24, 24, 32, 32]
    assert variant_of(25, True, "photometric", 0) == ("photometric", 32, True, 0)      # the variant whose choice exists in the twin only
    assert variant_of(9, False, "geometric", 0) == ("geometric", 16, False, 0) and init_variant_of(17, False, 2) == (24, False, 2)
    for mode in ("geometric", "prior"):
        with pytest.raises(ValueError):
            variant_of(8, True, mode, 1)
    upd, ini = run_variants(20, True, "photometric", 2)
    assert upd == {("photometric", 24, True, s) for s in (0, 1, 2)} and ini == {(24, True, 2)}
    assert run_variants(20, False, "prior", 1) == ({("prior", 24, False, 0)}, {(24, False, 1)})


def test_named_lists_reach_every_variant():
    upd, ini = q8c.named_variants()
    assert upd["a"] == ALL_UPDATE_VARIANTS, sorted(ALL_UPDATE_VARIANTS - upd["a"])
    assert ini["c"] == ALL_INIT_VARIANTS, sorted(ALL_INIT_VARIANTS - ini["c"])
    assert set().union(*upd.values()) == ALL_UPDATE_VARIANTS and set().union(*ini.values()) == ALL_INIT_VARIANTS
    # the per-pass launches visit every bucket, and the states the variant that only the twin keeps in another form
    assert {v[1] for v in upd["b"]} == {8, 16, 24, 32}
    assert ("photometric", 32, True, 0) in upd["d"] and ("prior", 8, True, 0) in upd["d"]


def census(n):
    """(update variant -> cases that launch it, init variant -> cases, (V, quantize) drawn) over the cases 0 .. n - 1"""
    upd, ini, drawn = {}, {}, set()
    for k in range(n):
        c = fuzz_common.draw(k)
        drawn.add((c.V, c.quantize))
        runs = [("photometric", c.max_scale)] + [("geometric", c.max_scale)] * (c.mode >= 1) + [("prior", c.max_scale)] * (c.mode == 2)
        for mode, max_scale in runs:
            u, i = run_variants(c.V, c.quantize, mode, max_scale)
            for v in u:
                upd.setdefault(v, set()).add(k)
            for v in i:
                ini.setdefault(v, set()).add(k)
    return upd, ini, drawn


def census_holds(n):
    upd, ini, drawn = census(n)
    return (all(len(upd.get(v, ())) >= 2 for v in ALL_UPDATE_VARIANTS) and all(len(ini.get(v, ())) >= 1 for v in ALL_INIT_VARIANTS)
            and all((V, q) in drawn for V in q8c.EDGE_VIEWS for q in q8c.FORMATS))


def test_sweep_census():
    n = q8c.Q8_FUZZ_CASES
    assert n % 50 == 0 and n > 0
    upd, ini, drawn = census(n)
    few = {v: sorted(upd.get(v, ())) for v in ALL_UPDATE_VARIANTS if len(upd.get(v, ())) < 2}
    assert not few, f"update variants launched by fewer than two of {n} cases: {few}"
    assert not ALL_INIT_VARIANTS - set(ini), sorted(ALL_INIT_VARIANTS - set(ini))
    missing = [(V, q) for V in q8c.EDGE_VIEWS for q in q8c.FORMATS if (V, q) not in drawn]
    assert not missing, f"bucket edges never drawn in {n} cases: {missing}"
    assert not census_holds(n - 50), f"{n - 50} cases would do"
    print(f"\n{n} cases: every update variant in {min(len(s) for s in upd.values())} .. {max(len(s) for s in upd.values())} cases, "
          f"every init variant in {min(len(s) for s in ini.values())} .. {max(len(s) for s in ini.values())}")


@pytest.fixture(scope="module")
def tie_costs(pm, oracle):
    """(quantize, q8) -> [scale][V][H][W] of the oracle on the 32-view tie context, planes fronto-parallel at depth 3"""
    out = {}
    for quantize in q8c.FORMATS:
        cams, imgs, prm = q8c.tie_problem(pm, 32, quantize)
        for q8 in (True, False):
            cpu = oracle.create()
            oracle.set_texture_q8(cpu, q8)
            cpu.set_views(cams, imgs)
            q8c.assert_tie_homographies(cpu, 32)
            out[quantize, q8] = np.stack([cpu.eval_ncc(prm, q8c.tie_planes(3.0), s) for s in (0, 1, 2)])
    return out


def test_tie_shifts_are_the_ones_meant():
    shifts = dict(q8c.TIE_SHIFTS)
    assert len(q8c.TIE_SHIFTS) == 16 and len(shifts) == 16
    for k in q8c.TIE_KS:
        assert shifts[k, 0] * 512 == 2 * k + 1 and shifts[k, 1] - shifts[k, 0] == 2.0 ** -12 == shifts[k, 0] - shifts[k, -1]
    for s in shifts.values():
        assert 0.0 <= s <= 1.0 and s * 4096 == int(s * 4096)       # 12 bits of fraction: a pixel index below 64 plus s is exact in fp32
        for x in (-20.0, 0.0, 52.0):
            assert float(np.float32(x) + np.float32(s)) == x + s
    # round-half-up and round-half-even part on the even k, at the tie itself
    for k in q8c.TIE_KS:
        a = np.float32(shifts[k, 0])
        up, even = np.floor(a * np.float32(256) + np.float32(0.5)), np.rint(a * np.float32(256))
        assert up == k + 1 and even == (k if k % 2 == 0 else k + 1)
    assert np.floor(np.float32(shifts[255, 0]) * np.float32(256) + np.float32(0.5)) / 256 == 1.0


@pytest.mark.parametrize("quantize", q8c.FORMATS)
def test_tie_relations_hold_on_the_q8_oracle(tie_costs, quantize):
    for s in (0, 1, 2):
        assert q8c.assert_tie_relations(tie_costs[quantize, True][s], 32, quantize) == (10 if quantize else 8)


@pytest.mark.parametrize("quantize", q8c.FORMATS)
def test_exact_fractions_tell_the_three_views_of_a_tie_apart(tie_costs, quantize):
    for s in (0, 1, 2):
        assert q8c.assert_tie_relations(tie_costs[quantize, False][s], 32, quantize, q8=False) == 8


def test_tie_costs_are_mostly_real_costs(tie_costs):
    for key, costs in tie_costs.items():
        assert np.isfinite(costs).all()
        for s in (0, 1, 2):
            assert (costs[s] == 2.0).mean() < 0.5, (key, s, float((costs[s] == 2.0).mean()))
