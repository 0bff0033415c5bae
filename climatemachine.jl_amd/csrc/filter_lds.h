// LDS budget of the element-filter kernels (filters.h) and the chunk rule of EngineBase::filter_apply
// that follows from it.  Plain C++ with no HIP in it: the kernels, the launcher and the host program
// tests/host/host_filter_lds.cpp include the same functions, so the figure a launch is sized by is the
// figure the kernel's arrays add up to (the kernels static_assert their static arrays against it).
//
// A work-group of k_apply_filter / k_apply_mp_filter stages two buffers of nfs * Np doubles in dynamic
// LDS next to its static arrays; static plus dynamic stays within the 64 KiB a work-group may claim
// without asking for more.  FilterIndices states are independent, so a filter on more states than that
// admits runs as several launches; the atmos targets couple their ATMOS_NS states and run as one.
#pragma once

namespace cmdg {

constexpr int ATMOS_NS = 5;  // rho, rho u[3], rho e
enum { FILTER_FAM_SPECTRAL = 0, FILTER_FAM_MASS_PRESERVING = 1, FILTER_FAM_TMAR = 2 };  // = CMDG_FILTER_*
constexpr int FILTER_LDS_LIMIT = 64 * 1024;
constexpr int FILTER_CHUNK_MAX = 16;

constexpr int filter_np(int NQ) { return NQ * NQ * NQ; }
constexpr int filter_nt(int NQ) { return ((filter_np(NQ) + 63) / 64) * 64; }  // work-group size

// doubles in the kernel's __shared__ arrays
constexpr int filter_static_doubles(int family, int NQ)
{
    return family == FILTER_FAM_SPECTRAL          ? 2 * NQ * NQ                      // sFh, sFv
           : family == FILTER_FAM_MASS_PRESERVING ? NQ * NQ + 3 * filter_nt(NQ)      // sF, sM, sB, sA
                                                  : 2 * 64;                          // sMJQ, sMJQc
}
// doubles of dynamic LDS a launch on nfs filtered states asks for
constexpr int filter_dynamic_doubles(int family, int NQ, int nfs)
{
    return family == FILTER_FAM_TMAR ? 0 : 2 * nfs * filter_np(NQ);
}
// bytes of LDS, static plus dynamic, of one work-group
constexpr int filter_lds_bytes(int family, int NQ, int nfs)
{
    return 8 * (filter_static_doubles(family, NQ) + filter_dynamic_doubles(family, NQ, nfs));
}
// the largest nfs <= FILTER_CHUNK_MAX whose work-group stays within FILTER_LDS_LIMIT (0: none does)
constexpr int filter_chunk(int family, int NQ)
{
    int nfs = FILTER_CHUNK_MAX;
    while (nfs > 0 && filter_lds_bytes(family, NQ, nfs) > FILTER_LDS_LIMIT) --nfs;
    return nfs;
}
// the rule before this header: min(16, 56 KiB / (16 Np)), which counted the dynamic buffers only
constexpr int filter_chunk_dynamic_only(int NQ)
{
    const int c = (56 * 1024) / (16 * filter_np(NQ));
    return c < 1 ? 1 : (c > FILTER_CHUNK_MAX ? FILTER_CHUNK_MAX : c);
}

// Atmos targets are launched unchunked: a chunk below ATMOS_NS would split them, and each part would
// run compute_filter_argument! / compute_filter_result! on all five states again.
template <int NQ>
constexpr bool filter_chunks_hold_atmos()
{
    return filter_chunk(FILTER_FAM_SPECTRAL, NQ) >= ATMOS_NS && filter_chunk(FILTER_FAM_MASS_PRESERVING, NQ) >= ATMOS_NS &&
           filter_chunk(FILTER_FAM_TMAR, NQ) >= 1;
}
static_assert(filter_chunks_hold_atmos<2>() && filter_chunks_hold_atmos<3>() && filter_chunks_hold_atmos<4>() &&
                  filter_chunks_hold_atmos<5>() && filter_chunks_hold_atmos<6>() && filter_chunks_hold_atmos<7>() &&
                  filter_chunks_hold_atmos<8>(),
              "filter chunk: an atmos target's five states must fit one launch at every compiled order");

}  // namespace cmdg
