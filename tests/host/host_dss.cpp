// The flatten-and-validate routine of direct stiffness summation (csrc/dss_tables.h) on the host:
// the tables of the reference's own test (test/Numerics/Mesh/DSS.jl: two elements side by side,
// N = (4, 4, 5)) written out as literals must flatten into the 30 node pairs of the shared face and
// sum as the reference does, and every malformed table must be refused with a reason.  Built by
// tests/test_dss_tables_host.py with -fsanitize=address,undefined and run as a process of its own.
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <string>
#include <vector>

#include "dss_tables.h"

using namespace cmdg;

static int failures = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                           \
        }                                                         \
    } while (0)

namespace {
constexpr int Q1 = 5, Q2 = 5, Q3 = 6, NP = Q1 * Q2 * Q3;
int64_t node(int i, int j, int k) { return 1 + i + Q1 * (j + Q2 * k); }

// what the topology of brickrange (0:2, 5:6, 0:1) holds (Topologies.jl:810-988)
struct Tables {
    std::vector<int64_t> vtconn{2, 1, 1, 2, 6, 1, 5, 2, 4, 1, 3, 2, 8, 1, 7, 2};
    std::vector<int64_t> vtconnoff{1, 1, 1, 5, 9, 9, 9, 9, 9, 13, 17, 17, 17};
    std::vector<int64_t> edgconn{6, 1, 1, 5, 1, 2, 8, 1, 1, 7, 1, 2, 10, 1, 1, 9, 1, 2, 12, 1, 1, 11, 1, 2};
    std::vector<int64_t> edgconnoff{1, 7, 13, 19, 25};
    std::vector<int64_t> fcconn{2, 1, 1, 2, 1};
    std::vector<int64_t> vertmap, edgemap, facemap;
    int64_t Nemax = 4, Nfmax = 12;
    cmdg_dss_desc d{};

    Tables()
    {
        // Grids.jl:640-745 for Nq = (5, 5, 6)
        for (int v = 0; v < 8; ++v) vertmap.push_back(node(v & 1 ? Q1 - 1 : 0, v & 2 ? Q2 - 1 : 0, v & 4 ? Q3 - 1 : 0));
        edgemap.assign((size_t)(Nemax * 12 * 2), -1);
        facemap.assign((size_t)(Nfmax * 6 * 2), -1);
        const int q[3] = {Q1, Q2, Q3};
        for (int dir = 0; dir < 3; ++dir)
            for (int e = 0; e < 4; ++e)
                for (int o = 0; o < 2; ++o)
                    for (int k = 0; k < q[dir] - 2; ++k) {
                        int ijk[3];
                        const int a = dir == 0 ? 1 : 0, b = dir == 2 ? 1 : 2;  // the two other directions
                        ijk[dir] = o ? q[dir] - 2 - k : 1 + k;
                        ijk[a] = e & 1 ? q[a] - 1 : 0;
                        ijk[b] = e & 2 ? q[b] - 1 : 0;
                        edgemap[(size_t)(k + Nemax * ((4 * dir + e) + 12 * o))] = node(ijk[0], ijk[1], ijk[2]);
                    }
        for (int dir = 0; dir < 3; ++dir)
            for (int side = 0; side < 2; ++side)
                for (int o = 0; o < 2; ++o) {
                    const int a = dir == 0 ? 1 : 0, b = dir == 2 ? 1 : 2;
                    int n = 0;
                    for (int kb = 1; kb < q[b] - 1; ++kb)
                        for (int ka = 1; ka < q[a] - 1; ++ka) {
                            int ijk[3];
                            ijk[dir] = side ? q[dir] - 1 : 0;
                            ijk[a] = o ? q[a] - 1 - ka : ka;
                            ijk[b] = kb;
                            facemap[(size_t)(n++ + Nfmax * ((2 * dir + side) + 6 * o))] = node(ijk[0], ijk[1], ijk[2]);
                        }
                }
        point();
    }
    void point()
    {
        d.Nq[0] = Q1, d.Nq[1] = Q2, d.Nq[2] = Q3;
        d.nelem = d.nreal = 2;
        d.nvt = (int64_t)vtconnoff.size() - 1, d.vtconn = vtconn.data(), d.vtconnoff = vtconnoff.data();
        d.nedg = (int64_t)edgconnoff.size() - 1, d.edgconn = edgconn.data(), d.edgconnoff = edgconnoff.data();
        d.nfc = 1, d.fcconn = fcconn.data();
        d.vertmap = vertmap.data();
        d.edgemap = edgemap.data(), d.Nemax = Nemax;
        d.facemap = facemap.data(), d.Nfmax = Nfmax;
    }
};

void refused(const char *what, const std::function<void(Tables &)> &spoil, const char *expect)
{
    Tables t;
    spoil(t);
    DssTables out;
    std::string err;
    const int r = dss_flatten(&t.d, out, err);
    if (r != CMDG_ERR_INVALID || err.find(expect) == std::string::npos) {
        printf("FAILED %s: status %d, message '%s' (expected '%s')\n", what, r, err.c_str(), expect);
        ++failures;
    }
}
}  // namespace

int main()
{
    {
        Tables t;
        DssTables f;
        std::string err;
        CHECK(dss_flatten(&t.d, f, err) == CMDG_OK);
        CHECK(err.empty());
        // the shared face has 5 x 6 nodes: 4 corners, 3 + 3 + 4 + 4 edge nodes, 12 interior
        CHECK(f.info[0] == 30 && f.info[1] == 60 && f.info[2] == 2 && f.info[3] == 60);
        CHECK(f.waves.size() == 1 && f.waves[0].n == 2 && f.waves[0].lanes == 30);
        CHECK(f.members.size() == 2 * DSS_WAVE);
        // faces first, their interior nodes on consecutive lanes, element 1 the first member
        for (int l = 0; l < 12; ++l) {
            CHECK(f.members[(size_t)l].elbase == 0 && f.members[(size_t)l].node == t.facemap[(size_t)(l + 12)] - 1);
            CHECK(f.members[(size_t)(DSS_WAVE + l)].elbase == NP && f.members[(size_t)(DSS_WAVE + l)].node == t.facemap[(size_t)l] - 1);
        }
        // values ldof + (e - 1) Np, three states: node (4, j, k) of element 1 meets node (0, j, k) of element 2
        const int ns = 3;
        std::vector<double> Q((size_t)(NP * ns * 2)), want;
        for (int e = 0; e < 2; ++e)
            for (int s = 0; s < ns; ++s)
                for (int n = 0; n < NP; ++n) Q[(size_t)(n + NP * (s + ns * e))] = (n + 1) + e * NP + 1000.0 * s;
        want = Q;
        for (int s = 0; s < ns; ++s)
            for (int k = 0; k < Q3; ++k)
                for (int j = 0; j < Q2; ++j) {
                    const size_t a = (size_t)(node(Q1 - 1, j, k) - 1 + NP * s), b = (size_t)(node(0, j, k) - 1 + NP * (s + ns));
                    want[a] = want[b] = Q[a] + Q[b];
                }
        dss_apply_host(f, Q.data(), ns);
        CHECK(Q == want);
    }
    refused("offsets that do not start at 1", [](Tables &t) { t.vtconnoff[0] = 0; }, "does not start at 1");
    refused("offsets that decrease", [](Tables &t) { t.vtconnoff[4] = 3; }, "vtconnoff decreases");
    refused("edge offsets that decrease", [](Tables &t) { t.edgconnoff[2] = 4; }, "edgconnoff decreases");
    refused("offsets that cut a record", [](Tables &t) { t.edgconnoff[1] = 6; }, "cuts a record");
    refused("an element out of range (vertex)", [](Tables &t) { t.vtconn[1] = 3; }, "names element 3");
    refused("an element out of range (edge)", [](Tables &t) { t.edgconn[2] = 0; }, "names element 0");
    refused("an element out of range (face)", [](Tables &t) { t.fcconn[3] = 3; }, "names element 3");
    refused("a node out of range (vertmap)", [](Tables &t) { t.vertmap[7] = NP + 1; }, "vertmap[7]");
    refused("a node out of range (edgemap)", [](Tables &t) { t.edgemap[0] = 0; }, "edgemap entry 0");
    refused("a node out of range (facemap)", [](Tables &t) { t.facemap[5] = -2; }, "facemap entry 5");
    refused("a local vertex out of range", [](Tables &t) { t.vtconn[0] = 9; }, "local vertex 9");
    refused("a local edge out of range", [](Tables &t) { t.edgconn[0] = 13; }, "local edge 13");
    refused("an edge orientation out of range", [](Tables &t) { t.edgconn[1] = 3; }, "orientation 3");
    refused("a local face out of range", [](Tables &t) { t.fcconn[2] = 7; }, "names face 7");
    refused("a face orientation out of range", [](Tables &t) { t.fcconn[4] = 2; }, "orientation 2");
    // vertex 2 of element 1 listed at a second unique vertex; an edge node that is a face node as well
    refused("a node in two groups (vertices)", [](Tables &t) { t.vtconn[4] = 2; }, "is in two groups");
    refused("a node in two groups (edge and face)", [](Tables &t) { t.edgemap[0 + 4 * 5] = t.facemap[0 + 12 * 1]; },
            "is in two groups");
    refused("too few points in the vertical", [](Tables &t) { t.d.Nq[2] = 2; }, "at least 3 points");
    refused("node numbers beyond 32 bits", [](Tables &t) { t.d.nelem = t.d.nreal = (int64_t)1 << 31; }, "32-bit");
    refused("a missing table", [](Tables &t) { t.d.fcconn = nullptr; }, "missing table");
    if (failures) return 1;
    printf("host dss: ok\n");
    return 0;
}
