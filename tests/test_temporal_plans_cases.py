"""The restated launch plans of the channels-last temporal kernels and their case table (tests/temporal_plans.py), checked without a
GPU: the constants against the sources' text, the backward's chunk count against the library's workspace query, every regime
populated, the tables mixed or uniform as their kind says, and the size caps."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import temporal_plans as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "activesparseshifts-pytorch_amd", "csrc")
TORCH = {"u8": torch.uint8, "f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}


def _constants(name):
    """every `constexpr <type> kName = <value>;` of a source file, a value that names another constant resolved"""
    text = open(os.path.join(CSRC, name)).read()
    found = {}
    for key, value in re.findall(r"^constexpr\s+\w+\s+(k\w+)\s*=\s*([^;]+);", text, re.M):
        value = value.strip()
        found[key] = found[value] if value in found else int(value)
    return found, text


def test_the_constants_are_the_sources():
    frames, _ = _constants("shiftnd_frames.hip")
    learn, text = _constants("shiftnd_frames_learn.hip")
    common, _ = _constants("shiftnd_common.hpp")
    for key, value in TP.FRAMES.items():
        assert frames[key] == value, ("shiftnd_frames.hip", key, frames[key], value)
    for key, value in TP.LEARN.items():
        assert learn[key] == value, ("shiftnd_frames_learn.hip", key, learn[key], value)
    assert common["kThreads"] == TP.K_THREADS
    # the forward's grid target is the named constant, not a literal
    assert re.search(r"wanted = \(kWantWorkgroups \+ frames - 1\) / frames;", text)


def test_the_figures_checked_by_hand():
    """shapes whose plans were worked out on paper from the sources"""
    for M, steps in ((65, 2), (129, 4), (257, 8), (64, 1)):
        p = TP.backward_plan(1024, 2, M, 64, 2)
        assert (p["steps"], p["plan_rps"], p["rps"], p["rows_per_wg"]) == (steps, 32, 32, 32 * steps), (M, p)
        assert p["workspace_bytes"] == 1024 * p["chunks"] * 64 * 24
    p = TP.backward_plan(2, 3, 196, 5, 2)        # 10-byte rows: 2-byte pieces, 5 of them; the plan assumes one 16-byte piece
    assert (p["unit"], p["P"], p["rps"], p["plan_rps"], p["steps"], p["chunks"], p["iterations"]) == (2, 5, 51, 256, 1, 1, 4), p
    p = TP.active_forward_plan(3072, 2, 300, 5, 2)
    assert (p["rps"], p["wanted"], p["most"], p["chunks"], p["rows_per_wg"], p["batches"]) == (51, 1, 2, 1, 408, 2), p
    p = TP.active_forward_plan(3072, 2, 129, 64, 2)
    assert (p["unit"], p["rps"], p["chunks"], p["rows_per_wg"], p["batches"], p["last_tail"]) == (16, 32, 1, 256, 2, 1), p
    p = TP.forward_plan(2, 8, 49, 64, 2)         # the small suite's "several workgroups per frame": one batch each, `most` decides
    assert (p["decided"], p["batches"], p["rows_per_wg"], p["chunks"]) == ("most", 1, 256, 1), p
    p = TP.forward_plan(512, 1, 56 * 56, 64, 2)  # N * T = 512 frames of 56 x 56 x 64 fp16: `wanted` decides, two batches
    assert (p["decided"], p["fewest"], p["wanted"], p["most"], p["batches"]) == ("wanted", 7, 12, 13, 2), p
    # a base one element off: the piece is the element
    assert TP.piece(8, 2, 1)["unit"] == 2 and TP.piece(8, 2, 0)["unit"] == 16 and TP.piece(5, 2, 0)["unit"] == 2
    assert TP.piece(2112, 2, 0)["P"] == 264 and TP.piece(2112, 2, 0)["rps"] == 1


def test_every_row_covers_its_frame():
    """chunks workgroups of rows_per_wg rows hold the M rows, the last one at least one; whole batches in the two forwards"""
    rs = np.random.RandomState(5)
    for _ in range(2000):
        N, T, M, C = int(rs.randint(1, 7000)), int(rs.randint(1, 18)), int(rs.randint(1, 9000)), int(rs.randint(1, 600))
        es, off = int(rs.choice([1, 2, 4, 8])), int(rs.randint(0, 2))
        for kernel, plan in TP.PLANS.items():
            p = plan(N, T, M, C, es, off)
            assert (p["chunks"] - 1) * p["rows_per_wg"] < M <= p["chunks"] * p["rows_per_wg"], (kernel, N, T, M, C, es, off, p)
            assert 1 <= p["last_rows"] <= p["rows_per_wg"] and p["unit"] >= es and p["P"] * p["unit"] == C * es
            if kernel != TP.FB:
                assert p["rows_per_wg"] % (p["rps"] * TP.IN_FLIGHT[kernel]) == 0
            if kernel == TP.FF:
                assert p["batches"] <= 2, p       # kMaxRowGroups / kInFlight


def test_the_backward_plan_is_the_workspace_query():
    """N * chunks * C * 24 bytes, for the [C] table (SHIFTND_FRAMES) and the per-clip one (SHIFTND_CLIP_FRAMES)"""
    from torchshifts import abi
    L = abi.lib()
    shapes = [(c[2], c[3]) for c in TP.CASES if c[1] == TP.FB]
    shapes += [((n, 2, m, c), dt) for n in (1, 2, 1023, 1024, 2048) for m in (1, 64, 65, 257, 2049) for c, dt in ((64, "f16"), (5, "f16"), (3, "f32"), (1056, "f32"))]
    for (N, T, M, C), dt in shapes:
        x = torch.empty((N, C, T, M), dtype=TORCH[dt], device="meta")
        for flags in (dict(frames=True), dict(clip_frames=True)):
            for pad, active in ((0, 0), (3, 1)):
                p = abi.problem(x, pad, active, None, shift_dim0=True, **flags)
                got = int(L.shiftnd_backward_workspace_bytes(ctypes.byref(p)))
                assert got == TP.backward_plan(N, T, M, C, TP.ES[dt])["workspace_bytes"], ((N, T, M, C), dt, flags, got)


def test_every_regime_holds_for_a_case():
    for regime in TP.REGIMES:
        rows = [c for c in TP.CASES if c[0] == regime]
        assert rows, regime
        for c in rows:
            assert TP.holds(regime, c), (regime, c, TP.plan_of(c))


def test_the_required_regimes_are_in_the_table():
    """the regimes the table exists for, read off each row's plan and not off the row's name"""
    plans = [(c, TP.plan_of(c)) for c in TP.CASES]
    ff = [(c, p) for c, p in plans if c[1] == TP.FF]
    fa = [(c, p) for c, p in plans if c[1] == TP.FA]
    fb = [(c, p) for c, p in plans if c[1] == TP.FB]
    two = [(c, p) for c, p in ff if p["batches"] == 2 and c[5].endswith(("pieces", "runs"))]
    assert {p["unit"] for c, p in two} == {1, 2, 4, 8, 16}
    in_flight = TP.FRAMES["kInFlight"]
    assert any(p["rows"] == 2 * in_flight * p["rps"] for c, p in two) and any(p["last_batches"] == 2 and p["last_tail"] < p["rps"] for c, p in two)
    assert any(p["wanted"] < p["fewest"] for c, p in ff) and any(p["fewest"] < p["wanted"] < p["most"] for c, p in ff)
    assert any(p["P"] > 256 and p["chunks"] > 1 for c, p in ff) and any(256 % p["P"] and p["batches"] == 2 for c, p in two)
    assert any(c[5] == "specials" and p["epp"] > 1 and p["rows_per_wg"] > p["rps"] for c, p in ff)
    for kinds in (("pieces",), ("runs",), ("specials",)):
        seen = {min(p["batches"], 3) for c, p in fa if c[5] in kinds and (kinds != ("specials",) or p["epp"] > 1)}
        assert seen >= {1, 2, 3}, (kinds, seen)
    assert any(p["wanted"] < p["most"] and p["last_rows"] < p["rows_per_wg"] and p["chunks"] > 1 for c, p in fa)
    assert any(p["unit"] < 16 and p["batches"] >= 2 for c, p in fa)
    # the unsuffixed kernels (16-byte pieces of several elements) past the first batch / the first row step, not their ragged forms alone
    whole = [(c, p) for c, p in fa if p["unit"] == 16 and p["epp"] > 1 and p["batches"] >= 2]
    assert any(c[5] in ("pieces", "runs") for c, p in whole) and any(c[5] == "specials" for c, p in whole)
    assert any(p["P"] == 8 and p["epp"] == 8 and c[5] == "pieces" for c, p in whole)       # 64 fp16 channels, the batched (uniform) path
    partial = [(c, p) for c, p in fb if p["chunks"] > 1 and p["last_rows"] < p["rows_per_wg"]]
    assert {p["steps"] for c, p in partial} == {1, 2, 4, 8}
    assert {p["steps"] for c, p in partial if p["unit"] == 16 and p["epp"] > 1} >= {2, 4, 8}
    ragged = [(c, p) for c, p in fb if p["rps"] != p["plan_rps"] and p["iterations"] >= 2]
    assert {p["unit"] for c, p in ragged} >= {2, 4, 8} and any(p["steps"] > 1 for c, p in ragged)
    assert any(p["P"] > 256 and p["steps"] > 1 for c, p in fb)
    for clip in (False, True):
        assert any(c[5].startswith("clip-") == clip and p["chunks"] > 1 and c[2][0] > 1 for c, p in fb), clip


def test_the_tables_are_what_their_kind_says():
    """ "pieces": no piece mixed; "runs": at most the two pieces at the run boundaries; "specials" on pieces of several elements: mixed
    pieces under both paddings; the rows of a per-clip table all differ from their neighbours"""
    for c in TP.unique_cases():
        kind = c[5].replace("clip-", "")
        actives = {TP.FF: (0,), TP.FA: (1,), TP.FB: (0, 1)}[c[1]]
        for pad in (0, 3):
            w = TP.table_of(c, pad)
            assert np.array_equal(w * 4, np.round(w * 4)) and np.abs(w).max() <= 2 * c[2][1] + 2, c
            if c[5].startswith("clip-"):
                assert w.shape == (c[2][0], c[2][3]) and (w[1:] != w[:-1]).any(axis=1).all(), c
            else:
                assert w.shape == (c[2][3],), c
            for active in actives:
                mixed, of = TP.mixed_pieces(c, pad, active)
                if kind == "pieces":
                    assert mixed == 0, (c, pad, active, mixed, of)
                elif kind == "runs":
                    assert mixed <= 2 < of, (c, pad, active, mixed, of)
                elif TP.plan_of(c)["epp"] > 1:
                    assert mixed >= 1, (c, pad, active, mixed, of)


def test_the_size_caps():
    for c in TP.CASES:
        assert c[6] == TP.nbytes(c) <= TP.CASE_CAP, c
    assert sum(TP.nbytes(c) for c in TP.unique_cases()) < TP.TOTAL_CAP
    assert sum(c[6] for c in TP.CASES) < TP.TOTAL_CAP


def test_a_wrong_element_is_placed_in_its_workgroup():
    shape = (384, 2, 641, 24)
    p = TP.active_forward_plan(*shape, 2, 1)
    assert (p["rows_per_wg"], p["rps"], p["chunks"]) == (120, 10, 6)
    flat = np.ravel_multi_index((5, 1, 2 * 120 + 57, 7), shape)
    text = TP.locate(TP.FA, shape, 2, 1, flat)
    assert "(5, 1, 297, 7)" in text and "workgroup %d " % ((5 * 2 + 1) * 6 + 2) in text and "batch 1, slot 1" in text and "step 5" in text, text


@pytest.mark.parametrize("regime", ["fb-steps-1-partial", "fa-one-batch-uniform", "ff-long-rows-several-chunks"])
def test_the_search_finds_the_small_rows(regime):
    """the search itself, on the regimes it answers in a moment (a grid cut down to the row's own width)"""
    row = [c for c in TP.CASES if c[0] == regime][0]
    found = TP.search(regime, row[5], rows=[(row[2][3], row[3])])
    assert found[1:6] == row[1:6], (found, row)


# ---- the generator of tests/test_fuzz_temporal_gpu.py -----------------------------------------------------------------------------
def test_the_fuzz_cases_fit_their_box_and_reach_every_kernel_name():
    """every seed: the largest tensor at most 1 MiB, T in 1..17 (16 frame slots in place), and -- by the rule of the names, which the
    GPU test then asserts case by case -- every kernel name of the family"""
    sizes = set()
    for seed in TP.FUZZ_SEEDS:
        cases = TP.fuzz_cases(seed)
        assert len(cases) == TP.FUZZ_COUNT and cases == TP.fuzz_cases(seed)
        names = set()
        for c in cases:
            assert c["N"] * c["T"] * c["C"] * c["M"] * TP.ES[c["dt"]] <= TP.FUZZ_BYTES, c
            assert 1 <= c["T"] <= (16 if c["family"].startswith("inplace") else 17) and c["C"] >= 2 and c["M"] >= 2 and c["off"] in (0, 1), c
            names.update(TP.fuzz_kernels(c))
            sizes.add(((c["M"] if c["layout"] == "segment" else c["C"]) * TP.ES[c["dt"]]))
        assert set(TP.FUZZ_MUST_SEE) <= names, (seed, sorted(set(TP.FUZZ_MUST_SEE) - names))
        assert {c["family"] for c in cases} == {f[0] for f in TP.FUZZ_FAMILIES}
    # the residues: the fastest dim at, below and above 16 bytes, 4096 (P = 256) and 8192, and piece counts that do not divide 256
    assert {16, 4096, 8192} <= sizes and any(s < 16 for s in sizes) and any(4096 < s < 4200 for s in sizes)
    assert any(s % 16 == 0 and 256 % (s // 16) for s in sizes)
