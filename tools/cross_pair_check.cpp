// cd_pair (csrc/cross.hip) and dx_pair (csrc/duplex.hip) as HOST code against brute-force run(s, t) and duplex(s, t)
// written here from the definitions (catch_amd/filter/cross_dimer.py, cross_duplex.py), on a tile's layout built in
// plain memory of exactly the tile's size, so that the address sanitizer sees a read that leaves it.  No GPU, no
// Python.  Build and run (tools/README.md):
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined -ffunction-sections -Wl,--gc-sections \
//         tools/cross_pair_check.cpp -o cross_pair_check && ./cross_pair_check
// (the two files' extern "C" entries are compiled with them; nothing here refers to them, and --gc-sections drops them
// with their references into the rest of the library)
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../catch_amd/csrc/cross.hip"
#include "../catch_amd/csrc/duplex.hip"

static std::mt19937_64 rng(20260521);
static u32 below(u32 n) { return (u32)(rng() % n); }

static bool is_base(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }
static char complement(char c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : 0; }
static bool pairs(char x, char y) { return is_base(x) && is_base(y) && complement(x) == y; }

// the longest run of pairs(s[x + k], t[y - k])
static int brute_run(const std::string &s, const std::string &t) {
    int best = 0;
    for (int x = 0; x < (int)s.size(); ++x)
        for (int y = 0; y < (int)t.size(); ++y) {
            int n = 0;
            while (x + n < (int)s.size() && y - n >= 0 && pairs(s[x + n], t[y - n])) ++n;
            best = n > best ? n : best;
        }
    return best;
}

// -dg of a dinucleotide and the terminals, in hundredths of a kcal/mol: cross_duplex.py's table
static int brute_stack(char a, char b) {
    static const char *names[16] = {"AA", "TT", "AT", "TA", "CA", "TG", "GT", "AC", "CT", "AG", "GA", "TC", "CG", "GC", "GG", "CC"};
    static const int dg[16] = {100, 100, 88, 58, 145, 145, 144, 144, 128, 128, 130, 130, 217, 224, 184, 184};
    for (int i = 0; i < 16; ++i)
        if (names[i][0] == a && names[i][1] == b) return dg[i];
    abort();
}
static int brute_term(char c) { return c == 'G' || c == 'C' ? 98 : 103; }

// the maximum of stab over every stretch of n >= 2 pairs, maximal or not; 0 without one
static int brute_duplex(const std::string &s, const std::string &t) {
    int best = 0;
    for (int x = 0; x < (int)s.size(); ++x)
        for (int y = 0; y < (int)t.size(); ++y) {
            int stacks = 0;
            for (int n = 0; x + n < (int)s.size() && y - n >= 0 && pairs(s[x + n], t[y - n]); ++n) {
                if (n) {
                    stacks += brute_stack(s[x + n - 1], s[x + n]);
                    const int v = stacks - brute_term(s[x]) - brute_term(s[x + n]);
                    best = v > best ? v : best;
                }
            }
        }
    return best;
}

static u64 reversed(u64 x) {
    u64 r = 0;
    for (int i = 0; i < 64; ++i) r |= ((x >> i) & 1ull) << (63 - i);
    return r;
}

// one side of a tile, [plane][2 W words][RG_TILE], every other record's words random
template <int W> struct Side {
    std::vector<u64> pl;
    Side() : pl((size_t)3 * 2 * W * RG_TILE) {}
    void set(const std::string &s, u32 column, bool reverse) {
        for (u64 &x : pl) x = rng();
        for (int w = 0; w < 2 * W; ++w)
            for (int p = 0; p < 3; ++p) pl[(size_t)(p * 2 * W + w) * RG_TILE + column] = 0;
        for (int w = 0; w < W; ++w) {
            u64 x[3];
            cd_pack_word((const u8 *)s.data(), (u32)s.size(), w, &x[0], &x[1], &x[2]);
            for (int p = 0; p < 3; ++p)
                pl[(size_t)(p * 2 * W + (reverse ? W - 1 - w : w)) * RG_TILE + column] = reverse ? reversed(x[p]) : x[p];
        }
    }
};

static std::string random_record(u32 len) {
    std::string s(len, 'A');
    for (char &c : s) {
        const u32 k = below(100);
        c = "ACGT"[below(4)];
        if (k < 5) c = 'N';
        else if (k < 10) c = (char)(c + 32);        // lower case: no base
    }
    return s;
}

static std::string revcomp(const std::string &p) {
    std::string r(p.rbegin(), p.rend());
    for (char &c : r) c = complement(c);
    return r;
}

static long checks = 0, failures = 0;
static void expect(bool ok, const char *what, int W, const std::string &s, const std::string &t, int thr, int got, int truth) {
    ++checks;
    if (ok) return;
    if (++failures <= 20)
        fprintf(stderr, "%s W=%d t=%d: got %d, brute force %d\n  s=%s\n  t=%s\n", what, W, thr, got, truth, s.c_str(), t.c_str());
}

// both functions, both modes, a dozen thresholds, with s on the row side and t on the column side
template <int W> static void check_order(const std::string &s, const std::string &t) {
    static Side<W> row, col;
    static std::vector<u16> q((size_t)64 * W * RG_TILE);
    const u32 r = below(RG_TILE), lane = below(RG_TILE);
    row.set(s, r, false);
    col.set(t, lane, true);
    for (u16 &x : q) x = (u16)rng();
    dx_prefix<W>(&row.pl[r], &q[r]);
    const u64 *a = &row.pl[r], *rb = &col.pl[lane];
    const int la = (int)s.size(), lb = (int)t.size();
    const int run = brute_run(s, t), dup = brute_duplex(s, t);
    const int run_t[12] = {0, 1, 5, 20, 62, 63, 64, 65, run - 1 < 0 ? 0 : run - 1, run, run / 2, 64 * W + 1};
    for (int thr : run_t) {
        const int v = CdLength::pair<W, false>(a, rb, nullptr, la, lb, thr), f = CdLength::pair<W, true>(a, rb, nullptr, la, lb, thr);
        expect(run > thr ? v == run : v <= thr, "cd_pair<false>", W, s, t, thr, v, run);
        expect(run > thr ? (f > thr && f <= run) : f <= thr, "cd_pair<true>", W, s, t, thr, f, run);
    }
    const int dup_t[12] = {0, 1, 57, 63, 64, 223, 224, 1000, dup - 1 < 0 ? 0 : dup - 1, dup, dup / 2, 224 * 255 + 1};
    for (int thr : dup_t) {
        const int v = DxDuplex::pair<W, false>(a, rb, &q[r], la, lb, thr), f = DxDuplex::pair<W, true>(a, rb, &q[r], la, lb, thr);
        expect(dup > thr ? v == dup : v <= thr, "dx_pair<false>", W, s, t, thr, v, dup);
        expect(dup > thr ? (f > thr && f <= dup) : f <= thr, "dx_pair<true>", W, s, t, thr, f, dup);
    }
}

template <int W> static void check_words(int pairs_wanted) {
    const u32 maxlen = 64 * W;
    for (int i = 0; i < pairs_wanted; ++i) {
        // lengths: anything, with the ends of the range often
        u32 ls = below(8) == 0 ? maxlen - below(2) : below(maxlen + 1), lt = below(8) == 0 ? maxlen - below(2) : below(maxlen + 1);
        if (below(40) == 0) ls = below(3);
        std::string s = random_record(ls), t = random_record(lt);
        const u32 room = ls < lt ? ls : lt;
        const u32 kind = below(4);                  // 0: nothing planted
        if (kind && room >= 2) {
            const u32 k = 2 + below(room - 1 < 80 ? room - 1 : 80);
            const std::string piece = [&] { std::string p(k, 'A'); for (char &c : p) c = "ACGT"[below(4)]; return p; }();
            u32 os = below(ls - k + 1), ot = below(lt - k + 1);
            if (kind == 2 && ls > 64) os = 64 - k / 2 + k <= ls ? 64 - k / 2 : ls - k;     // across the word edge 63 | 64
            if (kind == 3) { os = ls - k; if (below(2)) ot = lt - k; }                     // up to the last character
            s.replace(os, k, piece);
            t.replace(ot, k, revcomp(piece));
        }
        check_order<W>(s, t);
        check_order<W>(t, s);
    }
}

int main() {
    check_words<1>(1500);
    check_words<2>(1500);
    check_words<4>(1200);
    printf("cross_pair_check: %ld comparisons, %ld failures\n", checks, failures);
    return failures ? 1 : 0;
}
