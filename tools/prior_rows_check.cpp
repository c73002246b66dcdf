// prior_rows_check.cpp -- the row bound of the planar prior's task table (pm::prior_rows, csrc/pm_prior.hpp: the rows
// mpmvs_prior_from_triangles dispatches per triangle) against the loop it has to cover, written out literally:
//     float L = sqrt(e);  float step = 1.0 / L;  for (float p = 0; p < 1.0; p += step) ++rows;        (reference src/PatchMatch.cpp:557-564)
// over  every e below 2^20, and the first and last e of every run of equal floor(L) up to the edge from which the bound counts the
//       loop itself (the count never falls as e grows: a larger e has a smaller or equal step, and fp32 addition is monotone);
//       every integer L in 1 .. 65 535;
//       100 000 seeded e below 2 * 65 535^2, the largest squared edge an image can hold (both sides at most 65 535).
// The bound must never be below the loop's count and never a task (64 rows) or more above it, and refuse e outside [0, 2 * 65535^2].  Also prints where the loop first
// outruns floor(L) + 3 rows, and that bound in whole tasks: what the table covered before.
// Includes the header without HIP; a host program, so that it runs under the sanitizers:
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Imp-mvs_amd/csrc \
//       -o build/prior_rows_check tools/prior_rows_check.cpp && build/prior_rows_check
// Prints one line per range and "all covered"; exit status 1 on any miss.  `prior_rows_check N` thins the last two ranges to every
// N-th integer L and 100 000 / N drawn e (tests/test_prior_sweep_cpu.py runs it so; the full ranges take a quarter of a minute).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "pm_prior.hpp"

static int literal_rows(long long e) {
    const float L = (float)std::sqrt((double)e);
    const float step = (float)(1.0 / L);
    int rows = 0;
    for (float p = 0; p < 1.0; p += step) ++rows;
    return rows;
}

struct Range {
    const char* name;
    long long n = 0, below = 0, far = 0;           // entries; bound < count; bound >= count + 64
    long long lowest = 1 << 30, highest = -(1 << 30);   // count - floor(L)
    int slack = 0;                                 // largest bound - count
    long long first_over_rows = -1, first_over_tasks = -1;   // smallest e whose count exceeds floor(L) + 3 / that in whole tasks
    void take(long long e) {
        const int want = literal_rows(e), got = pm::prior_rows(e);
        const long long fl = (long long)std::sqrt((double)e);
        ++n;
        below += got < want;
        far += got >= want + pm::kPriorTaskRows;
        slack = std::max(slack, got - want);
        lowest = std::min(lowest, want - fl);
        highest = std::max(highest, want - fl);
        const long long tasks = (fl + 3 + pm::kPriorTaskRows - 1) / pm::kPriorTaskRows * pm::kPriorTaskRows;
        if (want > fl + 3 && (first_over_rows < 0 || e < first_over_rows)) first_over_rows = e;
        if (want > tasks && (first_over_tasks < 0 || e < first_over_tasks)) first_over_tasks = e;
    }
    bool report() const {
        printf("%-34s %8lld entries: below the loop %lld, a task or more above %lld, largest surplus %d rows; loop - floor(L) in [%lld, %lld]", name, n, below, far,
               slack, lowest, highest);
        if (first_over_rows >= 0) printf("; first above floor(L) + 3 at L = %.2f", std::sqrt((double)first_over_rows));
        if (first_over_tasks >= 0) printf(", above its whole tasks at L = %.2f", std::sqrt((double)first_over_tasks));
        printf("\n");
        return below == 0 && far == 0;
    }
};

int main(int argc, char** argv) {
    const int thin = argc > 1 ? std::max(1, std::atoi(argv[1])) : 1;
    bool ok = true;
    Range all{"every e below 2^20"};
    for (long long e = 0; e < (1ll << 20); ++e) all.take(e);
    ok = all.report() && ok;
    Range ends{"ends of the runs of floor(L)"};
    long long last = 0;
    while ((last + 1) * (last + 1) <= pm::kPriorExactFrom) ++last;
    for (long long L = 1; L <= last + 1; ++L) {
        ends.take(L * L);
        ends.take((L + 1) * (L + 1) - 1);
    }
    ends.take(pm::kPriorExactFrom - 1);
    ends.take(pm::kPriorExactFrom);
    ok = ends.report() && ok;
    Range whole{"every integer L in 1 .. 65535"};
    for (long long L = 65535; L >= 1; L -= thin) whole.take(L * L);
    ok = whole.report() && ok;
    Range drawn{"100000 e below 2 * 65535^2"};
    std::mt19937_64 rng(5640);
    std::uniform_int_distribution<long long> pick(0, 2ll * 65535 * 65535 - 1);
    for (int k = 0; k < 100000 / thin; ++k) drawn.take(pick(rng));
    ok = drawn.report() && ok;
    // total: the largest edge an image holds is counted, anything beyond or below is refused at once (from L ~ 3.4e7 on the loop never ends)
    const bool refused = pm::prior_rows(pm::kPriorMaxEdgeSq) == literal_rows(pm::kPriorMaxEdgeSq) && pm::prior_rows(pm::kPriorMaxEdgeSq + 1) == -1 &&
                         pm::prior_rows(10000000000000000ll) == -1 && pm::prior_rows(1ll << 62) == -1 && pm::prior_rows(-1) == -1;
    printf("edges outside [0, 2 * 65535^2]: %s\n", refused ? "refused" : "NOT refused");
    ok = refused && ok;
    printf(ok ? "all covered\n" : "NOT covered\n");
    return ok ? 0 : 1;
}
