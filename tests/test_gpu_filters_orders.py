"""The element filters on the device at every compiled order, against two statements at once: the twin
oracle (oracle/filter_oracle.c) bit for bit -- the existing contract -- and the independent restatement
(tests/filters_restatement.py: 40-digit matrices checked on the host, one dense long double contraction
per element and direction) node by node inside its rounding bound.  The case table is that of
tests/test_filters_restatement_host.py, which holds the oracle to the same bounds without a device:
  * k_apply_filter (exponential, Boyd-Vandeven, cutoff) at N = 1, 2, 5, 7 and k_apply_mp_filter at
    N = 1, 2, 4, 5, 7, each on FilterIndices (a strict subset with one index twice) and on both atmos
    targets, in every / horizontal / vertical direction; k_apply_tmar_filter at N = 1, 2, 5, 7;
  * a 3 x 1 x 3 brick with unequal element widths (9 elements: the tail of xcd_remap) and the
    Held-Suarez sphere (curved metrics) for the mass-preserving and TMAR filters at N = 2 and 5;
  * more filtered states than one launch stages: mass preserving at N = 7 with 9 of 11 states (two
    launches per direction, the unfiltered states bit-identical), spectral at N = 7 with 17 states
    (three launches), mass preserving at N = 6 with 11 states (the launch 1 KiB under the LDS limit).
Atmos targets: at N = 2 .. 6 the handle is the dry atmosphere's and the targets are the library's own;
at N = 1 and 7, where that engine is not compiled, the handle is the advection-diffusion law's, created on
an auxiliary state two columns of which the test has filled, and the target names those columns.
Ghost elements of a partitioned handle keep their bytes.  Needs a real MI355X: ``-m gpu``."""
import numpy as np
import pytest

from helpers import pseudo1d_setup
from test_filters_restatement_host import (CASES, build_case, case_id, check_against_restatement, is_identity,
                                           make_filter, untouched_states)

pytestmark = pytest.mark.gpu
EVERY = 0


def _gpu(torch, a):
    x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return x


@pytest.fixture(scope="module")
def handle(cm, torch):
    """One handle per (grid, order), created on the case table's own auxiliary state."""
    made = {}

    def get(c):
        key = c[:2]
        if key not in made:
            setup, grid, aux, _, _, _ = build_case(c)
            if c[0] == "brick":
                made[key] = cm.dgmodel.DGModel(setup, grid, state_auxiliary=aux.copy())
            else:
                law, d, dd = setup
                made[key] = cm.dgmodel.DGModel(law, grid, direction=d, diffusion_direction=dd,
                                               state_auxiliary=aux.copy())
        return made[key]

    yield get
    for dg in made.values():
        dg.close()


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_device_equals_oracle_and_sits_inside_the_restatement_bound(cm, oracle, torch, handle, c):
    F = cm.mesh.filters
    _, grid, aux, target, filt, Q0 = build_case(c)
    dg = handle(c)
    for direction in c[4]:
        Qo = Q0.copy()
        oracle.apply_filter(Qo, target, grid, filt, direction=direction, state_auxiliary=aux)
        Q = _gpu(torch, Q0.copy())
        F.apply(Q, target, dg, filt, direction=direction)
        Qg = Q.cpu().numpy()
        r = check_against_restatement("device", c, direction, Qg)
        print("%s direction %d: device error / bound %.3f, |device - oracle| max %.3e"
              % (case_id(c), direction, r, np.abs(Qg - Qo).max()))
        assert np.array_equal(Qg, Qo), (direction, np.abs(Qg - Qo).max())
        assert is_identity(c, direction) or not np.array_equal(Qg, Q0)
        for s in untouched_states(c):
            assert np.array_equal(Qg[:, s], Q0[:, s]), s


@pytest.mark.parametrize("N", [4, 2])
def test_ghost_elements_keep_their_bytes(cm, torch, N):
    """Rank 0 of 2: one filter of each family leaves the ghost elements as they were, and gives the real
    elements what the single-rank handle gives the same elements."""
    F = cm.mesh.filters
    law1, whole, _ = pseudo1d_setup(Ne=3, N=N)
    law, part, _ = pseudo1d_setup(Ne=3, N=N, rank=0, size=2)
    nr = part.nreal
    assert 0 < nr < part.nelem and whole.nreal == whole.nelem
    pos = {int(g): i for i, g in enumerate(whole.topology.globalelems)}
    rows = np.array([pos[int(g)] for g in part.topology.globalelems])
    assert np.array_equal(part.vgeo[:nr], whole.vgeo[rows[:nr]])
    rng = np.random.default_rng(N)
    Qw = 1.0 + 0.6 * rng.standard_normal((whole.nelem, 3, whole.Np))
    Qp = np.ascontiguousarray(Qw[rows])
    Qp[nr:] = 1e3 + np.arange(Qp[nr:].size, dtype=np.float64).reshape(Qp[nr:].shape) / 7   # distinct values
    dgw, dgp = cm.dgmodel.DGModel(law1, whole), cm.dgmodel.DGModel(law, part)
    for kind in ("exponential", "masspreserving", "tmar"):
        target = F.FilterIndices(3, 1)
        a, b = _gpu(torch, Qw), _gpu(torch, Qp)
        F.apply(a, target, dgw, make_filter(kind, whole), direction=EVERY)
        F.apply(b, target, dgp, make_filter(kind, part), direction=EVERY)
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert np.array_equal(b[nr:].view(np.uint64), Qp[nr:].view(np.uint64)), kind
        assert np.array_equal(b[:nr], a[rows[:nr]]), kind
        assert not np.array_equal(b[:nr, 0], Qp[:nr, 0]) and np.array_equal(b[:nr, 1], Qp[:nr, 1])
    dgw.close()
    dgp.close()
