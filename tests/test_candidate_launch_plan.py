"""The launch plans of the candidate rule kernels (csrc/rule_host.h: row_plan and plane_plan, through the test entry
point catchhip_selftest_candidate_plan) against the seven mirrors of the launch arithmetic that the rule tests keep,
for every candidate length from 1 to 4,096.  No GPU: the entry point is host arithmetic and takes no context.

The mirrors were written from the five launch sites that the one planner replaced, each next to the kernel test whose
lengths it justifies; they are imported from there, not copied.  What each family puts behind its rows or planes is
stated here once, as its entry point states it to the planner."""
import ctypes

import numpy as np
import pytest

import test_background_filter as tbf
import test_composition_filter as tcf
import test_design_filters as tdf
import test_quality_measure as tqm
import test_structure_filter as tsf
import test_tm_filter as ttf

LENGTHS = range(1, 4097)
COUNTER_BYTES = 64                 # triplet counters per row
TABLE_BYTES = 64                   # dinucleotide table per workgroup


@pytest.fixture(scope="module")
def plan():
    import __graft_entry__ as g
    g.build()
    from catch_amd import _lib
    fn = _lib.lib().catchhip_selftest_candidate_plan
    c_u32p = ctypes.POINTER(ctypes.c_uint32)

    def call(L, row_extra=0, wg_extra=0, tail_align=4, aligned16=True, plane_tail=0, plane_align=4):
        rows, planes = np.zeros(7, dtype=np.uint32), np.zeros(5, dtype=np.uint32)
        rc = fn(L, row_extra, wg_extra, tail_align, int(aligned16), plane_tail, plane_align,
                rows.ctypes.data_as(c_u32p), planes.ctypes.data_as(c_u32p))
        assert rc == 0
        r = dict(zip(("rows", "stage", "nchunk", "pitch_dw", "extra_off_dw", "tail_off_dw", "lds"), map(int, rows)))
        p = dict(zip(("W", "rows", "lds_planes", "tail_off_dw", "lds"), map(int, planes)))
        return r, p
    return call


def _check_rows(r, L, row_extra, wg_extra, tail_align):
    """What holds for every row plan, whatever the family: the geometry the kernels index by."""
    assert r["nchunk"] == (L + 30) // 16 and r["pitch_dw"] == 4 * r["nchunk"] + 1 and r["pitch_dw"] % 2 == 1
    assert r["rows"] in (256, 128, 64) and (r["stage"] or r["rows"] == 256)
    assert r["extra_off_dw"] == (r["rows"] * r["pitch_dw"] if r["stage"] else 0)
    assert r["tail_off_dw"] >= r["extra_off_dw"] + r["rows"] * row_extra // 4 and r["tail_off_dw"] * 4 % tail_align == 0
    assert r["lds"] == r["tail_off_dw"] * 4 + wg_extra and r["lds"] <= 65536


def test_row_plans_of_the_flag_kernels(plan):
    for L in LENGTHS:
        families = [(tdf._polya_workgroup(L), 0, 0), (tcf._composition_workgroup(L, False), 0, 0),
                    (tcf._composition_workgroup(L, True), COUNTER_BYTES, 0), (ttf._tm_workgroup(L), 0, ttf.TM_EXTRA),
                    (tbf._bg_workgroup(L), 0, tbf.BG_EXTRA)]
        for (rows, lds), row_extra, wg_extra in families:
            r, _ = plan(L, row_extra, wg_extra)
            assert (r["rows"], r["lds"]) == (rows, lds), (L, row_extra, wg_extra)
            assert r["stage"] == (lds > 256 * row_extra + wg_extra), (L, row_extra, wg_extra)
            _check_rows(r, L, row_extra, wg_extra, 4)


def test_row_plans_of_the_measure(plan):
    for L in LENGTHS:
        for W in (3, 64, 256):
            We = min(W, L) if L >= 4 else 0
            for histograms in (False, True):
                bins = (2 * (min(L, 1279) + 1) + (min(5 * (We - 2), 1279) + 1 if We else 1)) * 8 if histograms else 0
                for tm in (False, True):
                    row_extra, wg_extra = COUNTER_BYTES if We else 0, (TABLE_BYTES if tm else 0) + bins
                    r, _ = plan(L, row_extra, wg_extra, tail_align=8)
                    assert (r["rows"], bool(r["stage"])) == tqm._rows_workgroup(L, W, histograms, tm), (L, W, histograms, tm)
                    _check_rows(r, L, row_extra, wg_extra, 8)
                    # the bins lie behind the table, 8-byte aligned, as the launch places them
                    assert (r["tail_off_dw"] + (TABLE_BYTES if tm else 0) // 4) % 2 == 0


def test_plane_plans(plan):
    for L in LENGTHS:
        W = (L + 31) // 32
        _, p = plan(L)
        assert (p["rows"], p["lds"]) == tsf._structure_workgroup(L), L
        assert p["W"] == W and p["lds_planes"] == (p["lds"] > 0) and p["tail_off_dw"] * 4 == p["lds"]
        for histograms in (False, True):
            bins = 2 * (min(L, 1279) + 1) * 8 if histograms else 0
            _, p = plan(L, plane_tail=bins, plane_align=8)
            assert (p["rows"], p["lds"]) == tqm._structure_workgroup(L, histograms), (L, histograms)
            assert p["W"] == W and p["tail_off_dw"] % 2 == 0 and p["lds"] == p["tail_off_dw"] * 4 + bins <= 65536
            assert p["tail_off_dw"] == (p["rows"] * (6 * W + 7) if p["lds_planes"] else 0)


def test_rows_are_not_staged_from_an_unaligned_byte_array(plan):
    for L in (1, 100, 225, 226, 993, 994):
        for row_extra, wg_extra in ((0, 0), (COUNTER_BYTES, 0), (0, ttf.TM_EXTRA)):
            r, _ = plan(L, row_extra, wg_extra, aligned16=False)
            assert (r["rows"], r["stage"], r["extra_off_dw"], r["lds"]) == (256, 0, 0, 256 * row_extra + wg_extra)
