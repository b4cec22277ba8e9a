"""The poly(A) pre-filter on a synthetic dataset, end to end.  (GPU box)
    python tools/polya_profile.py S4 1.0 [--device-only]
Writes the groups as FASTA files and runs `catch_amd.design --filter-polya 20 4` on them: once to warm up, once timed
with the device front end (catchhip_candidates_drop_polya), once timed with CATCHHIP_HOST_FRONT_END=1 (the host's
strings).  Prints the wall times, the candidates the kernel saw and the bytes it moves for them.  Under
`rocprofv3 --kernel-trace --stats -- python tools/polya_profile.py S4 1.0 --device-only` the trace holds
polya_flag_kernel beside cand_hash_kernel of the same run."""
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from catch_amd import design, engine  # noqa: E402
from catch_amd.utils import synthetic  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "S2"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    device_only = "--device-only" in sys.argv[3:]
    groups = synthetic.dataset(name, scale=scale)
    tmp = tempfile.mkdtemp()
    files = []
    for gi, genomes in enumerate(groups):
        fn = os.path.join(tmp, "g%d.fasta" % gi)
        with open(fn, "w") as f:
            for j, g in enumerate(genomes):
                for c, s in enumerate(g):
                    f.write(">g%d_%d_%d\n%s\n" % (gi, j, c, s))
        files.append(fn)
    L = 100
    seen = []
    real = engine.Candidates.drop_polya

    def counted(self, *a):
        before = (self.ncandidates, self.n)
        real(self, *a)
        seen.append(before + (self.n,))
    engine.Candidates.drop_polya = counted

    def run(tag, host):
        out = os.path.join(tmp, tag + ".fasta")
        argv = files + ["-o", out, "-pl", str(L), "-ps", "50", "-m", "2", "-e", "50", "--filter-polya", "20", "4"]
        if host:
            os.environ["CATCHHIP_HOST_FRONT_END"] = "1"
        else:
            os.environ.pop("CATCHHIP_HOST_FRONT_END", None)
        t0 = time.perf_counter()
        design.main(design.parse_args(argv))
        el = time.perf_counter() - t0
        print("%s: %.3f s" % (tag, el), flush=True)
        return open(out, "rb").read()

    run("warm-up", False)
    del seen[:]
    dev = run("device front end", False)
    ncand, nuniq, nkept = (sum(s[i] for s in seen) for i in range(3))
    nchunk = (L + 30) // 16
    print("kernel calls %d: %d candidates, %d unique in, %d kept" % (len(seen), ncand, nuniq, nkept))
    print("polya_flag_kernel bytes: nuniq * (4 + 16 * %d + 4) = %d (upos, the rows' 16-byte chunks -- at most; "
          "flag)" % (nchunk, nuniq * (8 + 16 * nchunk)))
    print("cand_hash_kernel bytes: ncand * (4 + %d + 8 + 4) = %d (cpos, characters, key, value)"
          % (L, ncand * (L + 16)))
    if not device_only:
        host = run("host front end", True)
        print("same probes: %s" % (dev == host))


if __name__ == "__main__":
    main()
