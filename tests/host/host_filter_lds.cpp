// The LDS budget of the element-filter kernels (csrc/filter_lds.h) on the host: for every compiled
// order NQ = 2 .. 8 and every kernel family, the chunk EngineBase::filter_apply launches with keeps
// static plus dynamic LDS within 64 KiB, one state more would not (or the chunk is the cap of 16), an
// atmos target's five states fit one launch, and the rule that counted the dynamic buffers only is
// shown where it went over: the mass-preserving kernel at NQ = 8, 7 states, 70 144 B.  Prints the
// table.  Built by tests/test_filter_lds_host.py with -fsanitize=address,undefined and run as a
// process of its own.
#include <stdio.h>

#include "filter_lds.h"

using namespace cmdg;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                           \
        }                                                         \
    } while (0)

// the kernels' arrays, counted here by hand and not through filter_static_doubles
static int static_bytes_by_hand(int family, int NQ)
{
    const int Np = NQ * NQ * NQ, NT = (Np + 63) / 64 * 64;
    if (family == FILTER_FAM_SPECTRAL) return 8 * NQ * NQ + 8 * NQ * NQ;
    if (family == FILTER_FAM_MASS_PRESERVING) return 8 * NQ * NQ + 3 * 8 * NT;
    return 2 * 8 * 64;
}

int main()
{
    static_assert(filter_lds_bytes(FILTER_FAM_MASS_PRESERVING, 8, filter_chunk_dynamic_only(8)) == 70144,
                  "the figure of the rule that counted dynamic LDS only");
    static_assert(filter_lds_bytes(FILTER_FAM_MASS_PRESERVING, 7, filter_chunk(FILTER_FAM_MASS_PRESERVING, 7)) == 64488,
                  "N = 6 sits 1 KiB under the limit");
    const char *const name[3] = {"spectral", "mass-preserving", "TMAR"};
    printf("%-16s %3s %5s %6s %7s %8s %8s | %9s %9s\n", "family", "NQ", "Np", "chunk", "static", "dynamic", "total",
           "old chunk", "old total");
    for (int family = 0; family < 3; ++family)
        for (int NQ = 2; NQ <= 8; ++NQ) {
            const int Np = NQ * NQ * NQ, c = filter_chunk(family, NQ), old = filter_chunk_dynamic_only(NQ);
            const int st = 8 * filter_static_doubles(family, NQ), dy = 8 * filter_dynamic_doubles(family, NQ, c);
            const int total = filter_lds_bytes(family, NQ, c), old_total = filter_lds_bytes(family, NQ, old);
            printf("%-16s %3d %5d %6d %7d %8d %8d | %9d %9d%s\n", name[family], NQ, Np, c, st, dy, total, old, old_total,
                   old_total > FILTER_LDS_LIMIT ? "  <- over 64 KiB" : "");
            CHECK(filter_np(NQ) == Np && filter_nt(NQ) % 64 == 0 && filter_nt(NQ) >= Np && filter_nt(NQ) < Np + 64);
            CHECK(st == static_bytes_by_hand(family, NQ));
            CHECK(dy == (family == FILTER_FAM_TMAR ? 0 : 16 * c * Np));
            CHECK(total == st + dy && total <= FILTER_LDS_LIMIT);
            CHECK(c >= 1 && c <= FILTER_CHUNK_MAX);
            CHECK(c == FILTER_CHUNK_MAX || filter_lds_bytes(family, NQ, c + 1) > FILTER_LDS_LIMIT);
            CHECK(family == FILTER_FAM_TMAR || c >= ATMOS_NS);
            // every chunk size a launch can see stays within the limit, and the budget grows with nfs
            for (int nfs = 1; nfs <= c; ++nfs) {
                CHECK(filter_lds_bytes(family, NQ, nfs) <= FILTER_LDS_LIMIT);
                CHECK(filter_lds_bytes(family, NQ, nfs) <= filter_lds_bytes(family, NQ, nfs + 1));
            }
            // the chunk shrinks exactly where the old rule was over the limit; elsewhere it is the old
            // one, or larger where the old rule's 8 KiB of head room went unused
            const bool over = family == FILTER_FAM_MASS_PRESERVING && NQ == 8;
            CHECK((old_total > FILTER_LDS_LIMIT) == over && (c < old) == over);
            if (c > old) CHECK(NQ >= 7 && (family == FILTER_FAM_TMAR || filter_lds_bytes(family, NQ, old + 1) <= FILTER_LDS_LIMIT));
        }
    CHECK(filter_chunk_dynamic_only(8) == 7 && filter_chunk(FILTER_FAM_MASS_PRESERVING, 8) == 6);
    CHECK(filter_lds_bytes(FILTER_FAM_MASS_PRESERVING, 8, 7) == 57344 + 12800);
    CHECK(filter_lds_bytes(FILTER_FAM_MASS_PRESERVING, 8, 6) == 61952);
    CHECK(filter_chunk(FILTER_FAM_SPECTRAL, 8) == 7 && filter_chunk(FILTER_FAM_MASS_PRESERVING, 7) == 10);
    CHECK(filter_chunk(FILTER_FAM_SPECTRAL, 5) == 16);  // N = 4: the 21-state test runs as 16 + 5
    CHECK(filter_chunk(FILTER_FAM_SPECTRAL, 40) == 0);  // nothing fits: reported, not rounded up to 1
    if (failures) return 1;
    printf("host filter lds: ok\n");
    return 0;
}
