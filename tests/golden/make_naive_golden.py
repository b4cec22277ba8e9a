#!/usr/bin/env python3
"""Fixture of design_naively and its two filters (authoring container only).

Runs the LIVE reference (a checkout named by CATCH_REFERENCE: its package
`catch` and its bin/design_naively.py) and records, as data only, in
tests/golden/naive.json.gz:

  (a) pairs    ~400 string pairs over ACGTN, lengths 1-130 (equal and unequal,
               related by substitutions or shifts, unrelated, with N): k_lcf for
               k in {0, 1, 2, 3, 5} and, for equal lengths, mismatches_at_offset
               at every legal offset
  (b) filters  inputs, predicate parameters and the outputs of
               NaiveRedundantFilter and DominatingSetFilter as index lists in
               returned order, always with the exact predicate
               (prune_with_heuristic_and_anchor=False)
  (c) runs     bin/design_naively.py's main on a small FASTA this script builds
               (three Ebola records cut to 3 kb), the LCF factory patched to the
               exact branch; the printed counts

The reference evaluates its predicate pair by pair in Python; a pair of 100
bases costs about 15 ms, so the script takes several minutes.  Verdicts of the
reference's predicate are memoised by the two strings: both filters ask for the
same pairs.

    CATCH_REFERENCE=<reference checkout> python tests/golden/make_naive_golden.py
"""
import argparse
import contextlib
import gzip
import importlib.util
import io
import json
import os
import random
import sys
import tempfile

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ["CATCH_REFERENCE"]
sys.path.insert(0, REF)

from catch import probe  # noqa: E402
from catch.filter import candidate_probes, dominating_set_filter  # noqa: E402
from catch.filter import naive_redundant_filter as nrf  # noqa: E402
from catch.utils import longest_common_substring as lcs  # noqa: E402

EBOLA = os.path.join(HERE, "ebola_zaire_100.fasta.gz")
KS = (0, 1, 2, 3, 5)


def read_fasta(path, limit):
    recs, cur = [], None
    with gzip.open(path, "rt") as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                if len(recs) == limit:
                    break
                cur = [line[1:], []]
                recs.append(cur)
            elif cur is not None:
                cur[1].append(line)
    return [(h, "".join(parts)) for h, parts in recs]


class memoised:
    """The reference's predicate with its verdicts remembered by the two strings.  An object of a module-level
    class: the reference's BaseFilter.filter pickles the filter, predicate included, for its worker pool."""

    def __init__(self, fn=None, exact_lcf=None):
        self.fn, self.exact_lcf, self.seen = fn, exact_lcf, {}

    def __getstate__(self):
        assert self.exact_lcf is not None, "only the exact LCF predicate travels to a worker"
        return dict(fn=None, exact_lcf=self.exact_lcf, seen={})

    def __call__(self, a, b):
        if self.fn is None:
            self.fn = REAL_LCF(*self.exact_lcf, prune_with_heuristic_and_anchor=False)
        key = (a.seq_str, b.seq_str)
        if key not in self.seen:
            self.seen[key] = bool(self.fn(a, b))
        return self.seen[key]


REAL_LCF = nrf.redundant_longest_common_substring


# -- (a) ------------------------------------------------------------------
def pair_cases(rng):
    def rand(n, n_weight=0.0):
        return "".join(rng.choices("ACGTN", weights=[1, 1, 1, 1, n_weight], k=n))

    def mutate(s, subs):
        s = list(s)
        for j in rng.sample(range(len(s)), min(subs, len(s))):
            s[j] = rng.choice("ACGTN")
        return "".join(s)
    lengths = [1, 2, 3, 7, 20, 31, 40, 60, 63, 64, 65, 66, 100, 127, 128, 129, 130]
    pairs = []
    for i in range(400):
        kind = i % 8
        L = lengths[i % len(lengths)] if i % 3 else rng.randrange(1, 131)
        nw = (0.0, 0.15, 0.6)[rng.randrange(3)] if kind in (5, 6, 7) else 0.0
        a = rand(L, nw)
        if kind == 0:       # a few substitutions
            b = mutate(a, rng.randrange(0, 6))
        elif kind == 1:     # a shifted copy of equal length
            s = rng.randrange(0, L)
            b = (a[s:] + rand(s))[:L] if rng.random() < 0.5 else (rand(s) + a)[:L]
            b = mutate(b, rng.randrange(0, 3))
        elif kind == 2:     # unrelated, equal length
            b = rand(L)
        elif kind == 3:     # unequal length, related: a piece of a, or a with flanks
            if L > 1 and rng.random() < 0.5:
                lo = rng.randrange(0, L - 1)
                b = mutate(a[lo:rng.randrange(lo + 1, L + 1)], rng.randrange(0, 3))
            else:
                b = (rand(rng.randrange(0, 30)) + mutate(a, rng.randrange(0, 4)) + rand(rng.randrange(1, 30)))[:130]
        elif kind == 4:     # unequal length, unrelated
            b = rand(rng.randrange(1, 131))
        elif kind == 5:     # N in one
            b = mutate("".join(c if c != "N" else "A" for c in a), rng.randrange(0, 4))
        elif kind == 6:     # N in both, related
            b = mutate(a, rng.randrange(0, 4))
        else:               # N in both, unrelated, any lengths
            b = rand(rng.randrange(1, 131), nw)
        rec = dict(a=a, b=b, k_lcf={str(k): int(lcs.k_lcf(a, b, k)[0]) for k in KS})
        if len(a) == len(b):
            pa, pb = probe.Probe.from_str(a), probe.Probe.from_str(b)
            rec["mismatches_at_offset"] = [int(pa.mismatches_at_offset(pb, o)) for o in range(-(L - 1), L)]
        pairs.append(rec)
    return pairs


# -- (b) ------------------------------------------------------------------
def run_filters(name, strs, kind, params, fn):
    probes = [probe.Probe.from_str(s) for s in strs]
    index = {id(p): i for i, p in enumerate(probes)}
    out = {}
    for label, cls in (("nrf", nrf.NaiveRedundantFilter), ("dsf", dominating_set_filter.DominatingSetFilter)):
        out[label] = [index[id(p)] for p in cls(fn)._filter(list(probes))]
    sys.stderr.write("%s: %d probes -> nrf %d, dsf %d\n" % (name, len(strs), len(out["nrf"]), len(out["dsf"])))
    return dict(name=name, probes=strs, kind=kind, params=params, nrf=out["nrf"], dsf=out["dsf"])


def slice_candidates(records):
    best = None
    for start in range(0, 6000, 100):     # (the issue's slice has 232 candidates, 176 of them unique)
        cands = []
        for _, seq in records[:4]:
            cands += [p.seq_str for p in candidate_probes.make_candidate_probes_from_sequences(
                [seq[start:start + 1200]], probe_length=60, probe_stride=20)]
        if best is None:
            best = (start, cands)
        if len(cands) == 232 and len(set(cands)) == 176:
            return start, cands
    return best


def families(rng):
    """About 600 probes of 60 bases in a few dozen tight families, shuffled."""
    out = []
    for _ in range(36):
        root = "".join(rng.choices("ACGT", k=90))
        for _ in range(rng.randrange(8, 26)):
            s = rng.randrange(0, 31)
            m = list(root[s:s + 60])
            for j in rng.sample(range(60), rng.randrange(0, 4)):
                m[j] = rng.choice("ACGT")
            out.append("".join(m))
    rng.shuffle(out)
    return out


def filter_cases(rng, records):
    def lcf(m, t):
        return memoised(nrf.redundant_longest_common_substring(m, t, prune_with_heuristic_and_anchor=False))

    def shift(s, t, **kw):
        return nrf.redundant_shift_and_mismatch_count(shift=s, mismatch_thres=t, **kw)
    start, cands = slice_candidates(records)
    uniq = list(dict.fromkeys(cands))
    sys.stderr.write("slice at %d: %d candidates, %d unique\n" % (start, len(cands), len(uniq)))
    cases = []
    for m, t in ((2, 40), (0, 30)):
        fn = lcf(m, t)
        cases.append(run_filters("slice_unique_lcf_%d_%d" % (m, t), uniq, "lcf", [m, t], fn))
        cases.append(run_filters("slice_dups_lcf_%d_%d" % (m, t), cands, "lcf", [m, t], fn))
    cases.append(run_filters("slice_dups_default", cands, "default", [], None))
    cases.append(run_filters("slice_unique_shift_5_3", uniq, "shift", [5, 3], shift(5, 3)))
    cases.append(run_filters("slice_dups_shift_5_3", cands, "shift", [5, 3], shift(5, 3)))
    cases.append(run_filters("slice_unique_shift_5_12_slow", uniq[:90], "shift_slow", [5, 12], shift(5, 12)))
    small = uniq[:48]
    cases.append(run_filters("small_shift_Lm1_0", small, "shift", [59, 0], shift(59, 0)))
    cases.append(run_filters("small_shift_L_0", small, "shift", [60, 0], shift(60, 0)))
    cases.append(run_filters("small_lcf_2_Lp1", small, "lcf", [2, 61], lcf(2, 61)))
    cases.append(run_filters("small_lcf_0_1", small, "lcf", [0, 1], lcf(0, 1)))
    cases.append(run_filters("small_dups_lcf_0_Lp1", small[:10] + small[:10], "lcf", [0, 61], lcf(0, 61)))
    fam = run_filters("families_shift_5_3", families(rng), "shift", [5, 3], shift(5, 3))
    # the reference returns a Python set of ints as a list: picks beyond the table size come out of order
    assert fam["dsf"] != sorted(fam["dsf"]), "the dominating-set list of the family case is ascending"
    cases.append(fam)
    return cases


# -- (c) ------------------------------------------------------------------
def load_command():
    spec = importlib.util.spec_from_file_location("reference_design_naively", os.path.join(REF, "bin", "design_naively.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_cases(records, tmp):
    text = "".join(">%s\n%s\n" % (h, s[:3000]) for h, s in records[:3])
    path = os.path.join(tmp, "naive3.fasta")
    with open(path, "w") as f:
        f.write(text)
    command = load_command()
    real = REAL_LCF

    def factory(mismatches, lcf_thres, prune_with_heuristic_and_anchor=True):
        return memoised(exact_lcf=(mismatches, lcf_thres))
    nrf.redundant_longest_common_substring = factory
    runs = []
    try:
        for options in (["-nrf", "3", "80"], ["-dsf", "3", "80"], [], ["--add-reverse-complements"]):
            ns = argparse.Namespace(dataset=path, probe_length=100, probe_stride=50, naive_redundant_filter=None,
                                    dominating_set_filter=None, add_reverse_complements=False,
                                    limit_target_genomes=None, limit_target_genomes_randomly_with_replacement=None,
                                    print_analysis=False)
            it = iter(options)
            for o in it:
                if o in ("-nrf", "-dsf"):
                    pair = [int(next(it)), int(next(it))]
                    setattr(ns, "naive_redundant_filter" if o == "-nrf" else "dominating_set_filter", pair)
                else:
                    ns.add_reverse_complements = True
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                command.main(ns)
            sys.stderr.write("run %s: %s" % (options, buf.getvalue()))
            runs.append(dict(options=options, stdout=buf.getvalue(), count=int(buf.getvalue().strip())))
    finally:
        nrf.redundant_longest_common_substring = real
    return dict(fasta=text, probe_length=100, probe_stride=50, runs=runs)


def main():
    rng = random.Random(20240917)
    records = read_fasta(EBOLA, 4)
    data = dict(python=sys.version.split()[0])
    data["pairs"] = pair_cases(rng)
    sys.stderr.write("%d pairs\n" % len(data["pairs"]))
    data["filters"] = filter_cases(rng, records)
    with tempfile.TemporaryDirectory() as tmp:
        data["runs"] = run_cases(records, tmp)
    with gzip.GzipFile(os.path.join(HERE, "naive.json.gz"), "wb", mtime=0) as g:
        g.write(json.dumps(data, indent=0).encode())


if __name__ == "__main__":
    main()
