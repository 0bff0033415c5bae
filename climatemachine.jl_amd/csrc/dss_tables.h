// Direct stiffness summation: the host half.  The reference's tables (grid.topology.vtconn,
// vtconnoff, edgconn, edgconnoff, fcconn and grid.vertmap, edgemap, facemap; Topologies.jl:810-988,
// Grids.jl:640-745) are checked and flattened into one list of groups: a group is one shared mesh
// node -- a vertex, the k-th interior node of an edge, the j-th interior node of a face -- and its
// members are the copies of that node, as (element base, node in the element), in the order
// dss_vertex! / dss_edge! / dss_face! (DSS.jl:190-316) add them.  Entries the reference marks -1
// (mixed polynomial orders) are dropped here.
//
// Groups never share a node: that is what lets the kernel sum in place without atomics, so it is
// checked, with a bitmap over Np nelem, and a table that breaks it is refused.
//
// Group order is free (groups are disjoint), member order is not (it fixes the rounding).  The
// groups are laid out faces first, then edges, then vertices, each class sorted by member count
// (stably: the interior nodes of one face or edge stay consecutive), and cut into waves of at most
// WAVE groups of one member count, so that the lanes of a wave run the same number of trips.
//
// No HIP in this file: tests/host/host_dss.cpp builds it with the host compiler and sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/cmdg.h"

namespace cmdg {

constexpr int DSS_WAVE = 64;

struct DssMember {
    int32_t elbase, node;  // Np * element and node, both 0-based: Q[(elbase * nstate + s Np) + node]
};
struct DssWave {
    int64_t moff;     // first member slot: member j of lane l is at moff + j * DSS_WAVE + l
    int32_t n, lanes;  // members per group, groups (lanes in use)
};
struct DssTables {
    int Np = 0;
    int64_t nelem = 0;
    std::vector<DssWave> waves;
    std::vector<DssMember> members;  // padded to whole waves
    int64_t info[4] = {0, 0, 0, 0};  // groups, members, max members per group, nodes touched
};

// CMDG_OK, or CMDG_ERR_INVALID with the reason in err
inline int dss_flatten(const cmdg_dss_desc *d, DssTables &out, std::string &err)
{
    auto invalid = [&](const std::string &m) {
        err = "cmdg_dss_create: " + m;
        return (int)CMDG_ERR_INVALID;
    };
    auto str = [](int64_t v) { return std::to_string(v); };
    for (int k = 0; k < 3; ++k)
        if (d->Nq[k] < 2) return invalid("Nq[" + str(k) + "] is " + str(d->Nq[k]) + ": at least 2 points per direction");
    if (d->Nq[2] < 3) return invalid("the vertical needs at least 3 points (the reference has no maps below)");
    const int64_t Np = (int64_t)d->Nq[0] * d->Nq[1] * d->Nq[2];
    if (d->nelem < 0 || d->nreal < 0 || d->nreal > d->nelem) return invalid("nreal and nelem do not fit");
    if (d->nvt < 0 || d->nedg < 0 || d->nfc < 0 || d->Nemax < 0 || d->Nfmax < 0) return invalid("negative size");
    if ((double)Np * (double)d->nelem > 2147483647.0)
        return invalid("Np nelem = " + str(Np) + " x " + str(d->nelem) + " is beyond 32-bit node numbers");
    if (!d->vertmap || (d->nvt > 0 && (!d->vtconn || !d->vtconnoff)) ||
        (d->nedg > 0 && (!d->edgconn || !d->edgconnoff || !d->edgemap)) || (d->nfc > 0 && (!d->fcconn || !d->facemap)))
        return invalid("missing table");
    const int64_t nelem = d->nelem, Nemax = d->Nemax, Nfmax = d->Nfmax;
    // ---- the maps: node numbers 1..Np, or -1 in the edge and face maps
    for (int v = 0; v < 8; ++v)
        if (d->vertmap[v] < 1 || d->vertmap[v] > Np)
            return invalid("vertmap[" + str(v) + "] is " + str(d->vertmap[v]) + ", outside 1.." + str(Np));
    if (d->nedg > 0)
        for (int64_t i = 0; i < Nemax * 12 * 2; ++i)
            if (d->edgemap[i] != -1 && (d->edgemap[i] < 1 || d->edgemap[i] > Np))
                return invalid("edgemap entry " + str(i) + " is " + str(d->edgemap[i]) + ", outside 1.." + str(Np));
    if (d->nfc > 0)
        for (int64_t i = 0; i < Nfmax * 6 * 2; ++i)
            if (d->facemap[i] != -1 && (d->facemap[i] < 1 || d->facemap[i] > Np))
                return invalid("facemap entry " + str(i) + " is " + str(d->facemap[i]) + ", outside 1.." + str(Np));
    // ---- offsets: 1-based, monotone, whole records
    auto offsets = [&](const int64_t *off, int64_t n, int rec, const char *name) -> std::string {
        if (off[0] != 1) return std::string(name) + " does not start at 1";
        for (int64_t i = 0; i < n; ++i) {
            if (off[i + 1] < off[i]) return std::string(name) + " decreases at " + str(i);
            if ((off[i + 1] - off[i]) % rec) return std::string(name) + " cuts a record at " + str(i);
        }
        return std::string();
    };
    if (d->nvt > 0) {
        const std::string m = offsets(d->vtconnoff, d->nvt, 2, "vtconnoff");
        if (!m.empty()) return invalid(m);
    }
    if (d->nedg > 0) {
        const std::string m = offsets(d->edgconnoff, d->nedg, 3, "edgconnoff");
        if (!m.empty()) return invalid(m);
    }
    // ---- groups in the reference's order; goff[g] .. goff[g + 1] are the members of group g
    std::vector<DssMember> gm;
    std::vector<int64_t> goff(1, 0);
    std::vector<int64_t> nclass(3, 0);  // groups of faces, edges, vertices
    std::vector<uint8_t> seen((size_t)((Np * nelem + 7) / 8), 0);
    std::string dup;
    auto add = [&](int64_t el1, int64_t node1) {  // 1-based, checked by the caller
        const int64_t id = (el1 - 1) * Np + (node1 - 1);
        if (seen[id >> 3] & (1u << (id & 7))) {
            if (dup.empty()) dup = "node " + str(node1) + " of element " + str(el1) + " is in two groups";
        } else {
            seen[id >> 3] |= (uint8_t)(1u << (id & 7));
        }
        gm.push_back(DssMember{(int32_t)((el1 - 1) * Np), (int32_t)(node1 - 1)});
    };
    auto close_group = [&](int cls) {
        if ((int64_t)gm.size() > goff.back()) {
            goff.push_back((int64_t)gm.size());
            nclass[cls] += 1;
        }
    };
    // faces (dss_face!): facemap[j, lfc, ordr == 3 ? 2 : 1] of lel with facemap[j, nabrlfc, 1] of nabrlel
    for (int64_t fx = 0; fx < d->nfc; ++fx) {
        const int64_t lfc = d->fcconn[fx], lel = d->fcconn[fx + d->nfc], nfc = d->fcconn[fx + 2 * d->nfc],
                      nel = d->fcconn[fx + 3 * d->nfc], ordr = d->fcconn[fx + 4 * d->nfc];
        if (lfc < 1 || lfc > 6 || nfc < 1 || nfc > 6)
            return invalid("fcconn row " + str(fx) + " names face " + str(lfc < 1 || lfc > 6 ? lfc : nfc) + ", outside 1..6");
        if (lel < 1 || lel > nelem || nel < 1 || nel > nelem)
            return invalid("fcconn row " + str(fx) + " names element " + str(lel < 1 || lel > nelem ? lel : nel) +
                           ", outside 1.." + str(nelem));
        if (ordr != 1 && ordr != 3)
            return invalid("fcconn row " + str(fx) + " has orientation " + str(ordr) + ": 1 and 3 are what the mesh produces");
        const int64_t o = ordr == 3 ? 1 : 0;
        for (int64_t j = 0; j < Nfmax; ++j) {
            const int64_t loc1 = d->facemap[j + Nfmax * ((lfc - 1) + 6 * o)], loc2 = d->facemap[j + Nfmax * (nfc - 1)];
            if (loc1 != -1 && loc2 != -1) {
                add(lel, loc1);
                add(nel, loc2);
                close_group(0);
            }
        }
    }
    // edges (dss_edge!): for every k the members j = 1..nledg with edgemap[k, ledg, lor] != -1
    for (int64_t ex = 0; ex < d->nedg; ++ex) {
        const int64_t st = d->edgconnoff[ex] - 1, n = (d->edgconnoff[ex + 1] - d->edgconnoff[ex]) / 3;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t ledg = d->edgconn[st + 3 * j], lor = d->edgconn[st + 3 * j + 1], lel = d->edgconn[st + 3 * j + 2];
            if (ledg < 1 || ledg > 12) return invalid("edge " + str(ex) + " names local edge " + str(ledg) + ", outside 1..12");
            if (lor < 1 || lor > 2) return invalid("edge " + str(ex) + " has orientation " + str(lor) + ", outside 1..2");
            if (lel < 1 || lel > nelem)
                return invalid("edge " + str(ex) + " names element " + str(lel) + ", outside 1.." + str(nelem));
        }
        for (int64_t k = 0; k < Nemax; ++k) {
            for (int64_t j = 0; j < n; ++j) {
                const int64_t ledg = d->edgconn[st + 3 * j], lor = d->edgconn[st + 3 * j + 1], lel = d->edgconn[st + 3 * j + 2];
                const int64_t loc = d->edgemap[k + Nemax * ((ledg - 1) + 12 * (lor - 1))];
                if (loc != -1) add(lel, loc);
            }
            close_group(1);
        }
    }
    // vertices (dss_vertex!)
    for (int64_t vx = 0; vx < d->nvt; ++vx) {
        const int64_t st = d->vtconnoff[vx] - 1, n = (d->vtconnoff[vx + 1] - d->vtconnoff[vx]) / 2;
        for (int64_t j = 0; j < n; ++j) {
            const int64_t lvt = d->vtconn[st + 2 * j], lel = d->vtconn[st + 2 * j + 1];
            if (lvt < 1 || lvt > 8) return invalid("vertex " + str(vx) + " names local vertex " + str(lvt) + ", outside 1..8");
            if (lel < 1 || lel > nelem)
                return invalid("vertex " + str(vx) + " names element " + str(lel) + ", outside 1.." + str(nelem));
            add(lel, d->vertmap[lvt - 1]);
        }
        close_group(2);
    }
    if (!dup.empty()) return invalid(dup);
    // ---- layout: classes in order, each stably sorted by member count, cut into waves of one count
    const int64_t ngroups = (int64_t)goff.size() - 1;
    std::vector<int64_t> order((size_t)ngroups);
    for (int64_t g = 0; g < ngroups; ++g) order[g] = g;
    auto count = [&](int64_t g) { return goff[g + 1] - goff[g]; };
    int64_t c0 = 0;
    for (int cls = 0; cls < 3; ++cls) {
        std::stable_sort(order.begin() + c0, order.begin() + c0 + nclass[cls],
                         [&](int64_t a, int64_t b) { return count(a) < count(b); });
        c0 += nclass[cls];
    }
    out = DssTables();
    out.Np = (int)Np;
    out.nelem = nelem;
    int64_t maxn = 0;
    for (int64_t g0 = 0; g0 < ngroups;) {
        const int64_t n = count(order[g0]);
        int64_t g1 = g0 + 1;
        while (g1 < ngroups && g1 - g0 < DSS_WAVE && count(order[g1]) == n) ++g1;
        const int64_t moff = (int64_t)out.members.size();
        out.waves.push_back(DssWave{moff, (int32_t)n, (int32_t)(g1 - g0)});
        out.members.resize((size_t)(moff + n * DSS_WAVE), DssMember{0, 0});
        for (int64_t l = 0; l < g1 - g0; ++l)
            for (int64_t j = 0; j < n; ++j) out.members[(size_t)(moff + j * DSS_WAVE + l)] = gm[(size_t)(goff[order[g0 + l]] + j)];
        maxn = std::max(maxn, n);
        g0 = g1;
    }
    out.info[0] = ngroups;
    out.info[1] = (int64_t)gm.size();
    out.info[2] = maxn;
    out.info[3] = (int64_t)gm.size();  // groups are disjoint: every member is a node of its own
    return CMDG_OK;
}

// The summation on the host, group by group as the kernel does it: Q is (Np, nstate, nelem).
inline void dss_apply_host(const DssTables &t, double *Q, int nstate)
{
    for (const DssWave &w : t.waves)
        for (int l = 0; l < w.lanes; ++l)
            for (int s = 0; s < nstate; ++s) {
                double sum = -0.0;
                for (int j = 0; j < w.n; ++j) {
                    const DssMember m = t.members[(size_t)(w.moff + (int64_t)j * DSS_WAVE + l)];
                    sum += Q[(int64_t)m.elbase * nstate + (int64_t)s * t.Np + m.node];
                }
                for (int j = 0; j < w.n; ++j) {
                    const DssMember m = t.members[(size_t)(w.moff + (int64_t)j * DSS_WAVE + l)];
                    Q[(int64_t)m.elbase * nstate + (int64_t)s * t.Np + m.node] = sum;
                }
            }
}

}  // namespace cmdg
