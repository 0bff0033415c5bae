"""Shared builders for the tests (configurations of the reference's own tests)."""
import numpy as np

from cmdg_loader import cm

M = cm.mesh
BL = cm.balancelaws


def pseudo1d_setup(Ne=4, N=4, direction=0, flux_bc=False, rank=0, size=1, dim=3):
    """test/Numerics/DGMethods/advection_diffusion/pseudo1D_advection_diffusion.jl:293-368"""
    n = {0: np.ones(3) / np.sqrt(3), 1: np.array([1, 1, 0]) / np.sqrt(2),
         2: np.array([0, 0, 1.0])}[direction]
    rng = [np.linspace(-1, 1, Ne + 1)] * dim
    topl = M.StackedBrickTopology(rng, boundary=((1, 2),) * dim, periodicity=(False,) * dim,
                                  connectivity="full", rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = BL.AdvectionDiffusion(dim, BL.Pseudo1D(n, 1.0, 1 / 100, -1 / 2, 1 / 10),
                                (BL.InhomogeneousBC(0), BL.InhomogeneousBC(1)), flux_bc=flux_bc)
    dt = (1.0 / 4) / (Ne * N ** 2)
    dt = 1.0 / np.ceil(1.0 / dt)
    return law, grid, dt


def variable_degree_setup(level=1, orders=(4, 2), field="horizontal", rank=0, size=1):
    """variable_degree_advection_diffusion.jl:77-150 (dim = 3): polynomialorder = (N_h, N_v); its
    two equations are uncoupled (per-equation wave speed and diffusion tensor), so each is run
    as the one-equation Pseudo1D problem along n_hd = (1, 1, 0)/sqrt(2) or n_vd = (0, 0, 1);
    the operator works in every direction."""
    Ne = 2 ** (level - 1) * 4
    n = np.array([1, 1, 0]) / np.sqrt(2) if field == "horizontal" else np.array([0, 0, 1.0])
    rng = [np.linspace(-1, 1, Ne + 1)] * 3
    topl = M.StackedBrickTopology(rng, boundary=((1, 2),) * 3, periodicity=(False,) * 3,
                                  connectivity="full", rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, (orders[0], orders[0], orders[1]))
    law = BL.AdvectionDiffusion(3, BL.Pseudo1D(n, 1.0, 1 / 100, -1 / 2, 1 / 10),
                                (BL.InhomogeneousBC(0), BL.InhomogeneousBC(1)))
    dt = (1.0 / 4) / (Ne * max(orders) ** 2)
    return law, grid, dt


def rel_linf(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def periodic_hyperdiffusion_setup(Ne=4, N=4, direction=0, rank=0, size=1):
    """test/Numerics/DGMethods/advection_diffusion/periodic_3D_hyperdiffusion.jl:107-322"""
    from fractions import Fraction as Fr
    D = np.array([[9, 3, 5], [3, 7, 4], [5, 4, 10]], dtype=np.float64) / 50 / 100
    x = np.linspace(0.0, 2 * np.pi, Ne + 1)
    topl = M.StackedBrickTopology([x] * 3, periodicity=(True,) * 3, connectivity="full",
                                  rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = BL.AdvectionDiffusion(3, BL.ConstantHyperDiffusion(3, direction, D), (),
                                advection=False, diffusion=False, hyperdiffusion=True)
    dx = M.grids.min_node_distance(grid)
    dt = dx ** 4 / 25 / D.sum()
    dt = 1.0 / np.ceil(1.0 / dt)
    return law, grid, dt


def isentropic_vortex_setup(level=1, N=4, rank=0, size=1):
    """test/Numerics/DGMethods/Euler/isentropicvortex.jl:308-370 (dims = 3, DryModel,
    NoReferenceState, NoOrientation, ConstantDynamicViscosity(0), periodic BrickTopology)."""
    A = cm.atmos
    ps = A.PlanetParameters()
    setup = A.IsentropicVortexSetup(ps)
    L = setup.domain_halflength
    numelems = (2 ** (level - 1) * 5, 2 ** (level - 1) * 5, 1)
    rng = [np.linspace(-L, L, n + 1) for n in numelems]
    topl = M.BrickTopology(rng, periodicity=(True,) * 3, connectivity="face", rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = A.DryAtmosModel(setup, orientation=A.ORIENT_NONE, ref_state=None, viscosity=0.0,
                          dynamic_viscosity=True, sources=0, boundary_conditions=(),
                          param_set=ps)
    timeend = 2 * L / 10 / setup.translation_speed
    elementsize = min(2 * L / n for n in numelems)
    cs = np.sqrt(ps.cp_d / ps.cv_d * ps.R_d * setup.T_inf)
    dt = elementsize / cs / N ** 2
    nsteps = int(np.ceil(timeend / dt))
    dt = timeend / nsteps
    return law, grid, dt, timeend, nsteps


def held_suarez_setup(n_horz=3, n_vert=2, N=4, rank=0, size=1):
    """experiments/AtmosGCM/heldsuarez.jl:174-240 with AtmosGCMConfiguration
    (src/Driver/driver_configs.jl:344-470): stacked cubed sphere, radii [a, a + 30 km],
    boundary (1, 2), equiangular warp, Rusanov + central fluxes, DryBiharmonic(8 h),
    ConstantKinematicViscosity(0), sources (Gravity, Coriolis, HeldSuarezForcing),
    diffusion direction horizontal.  Returns (law, grid, direction, diffusion_direction)."""
    A = cm.atmos
    ps = A.PlanetParameters()
    a, H = ps.planet_radius, 30e3
    Rrange = np.linspace(a, a + H, n_vert + 1)
    topl = M.StackedCubedSphereTopology(n_horz, Rrange, boundary=(1, 2), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)
    law = A.DryAtmosModel(A.HeldSuarezSetup(ps), orientation=A.ORIENT_SPHERICAL,
                          ref_state=A.DecayingTemperatureProfile(ps, 290.0, 220.0, 8e3),
                          viscosity=0.0, dynamic_viscosity=False,
                          hyperdiffusion_timescale=8 * 3600.0,
                          sources=A.SRC_GRAVITY | A.SRC_CORIOLIS | A.SRC_HELD_SUAREZ,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT),
                          param_set=ps)
    return law, grid, 0, 1


def courant_test_setup(Neh=10, Nev=4, N=4, rank=0, size=1):
    """test/Numerics/DGMethods/courant.jl:63-135 (dim = 3): stacked brick [0,1]^2 x [1,2],
    FlatOrientation, NoReferenceState, ConstantDynamicViscosity(2), Gravity source."""
    A = cm.atmos
    ps = A.PlanetParameters()
    rng = [np.linspace(0.0, 1.0, Neh + 1), np.linspace(0.0, 1.0, Neh + 1),
           np.linspace(1.0, 2.0, Nev + 1)]
    topl = M.StackedBrickTopology(rng, connectivity="full", rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    setup = A.CourantTestSetup(ps)
    law = A.DryAtmosModel(setup, orientation=A.ORIENT_FLAT, ref_state=None, viscosity=2.0,
                          dynamic_viscosity=True, sources=A.SRC_GRAVITY,
                          boundary_conditions=(), param_set=ps)
    return law, grid, setup


def rising_bubble_setup(nx=20, ny=1, nz=20, N=4, rank=0, size=1):
    """experiments/TestCase/risingbubble.jl:93-132,186-200 through AtmosLESConfiguration
    (src/Driver/driver_configs.jl:190-290): stacked brick [0,10 km] x [0,500 m] x [0,10 km]
    with 500 m elements (resolution 125 m x N = 4), periodic in x and y, boundary (1, 2) in
    z with the default AtmosBC, FlatOrientation, HydrostaticState(DryAdiabaticProfile(300 K)),
    SmagorinskyLilly(C_smag), DryModel, Gravity; Rusanov + central fluxes.
    BASELINE config 2 is the same setup at 20 x 20 x 20 elements."""
    A = cm.atmos
    ps = A.PlanetParameters()
    rng = [np.linspace(0.0, 500.0 * nx, nx + 1), np.linspace(0.0, 500.0 * ny, ny + 1),
           np.linspace(0.0, 500.0 * nz, nz + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False),
                                  boundary=((0, 0), (0, 0), (1, 2)), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    # the reference's bubble (centre 5 km, 2 km; radius 2 km) on the full 10 km domain; scaled
    # with the domain on the reduced meshes of the tests so that it stays inside
    Lx, Lz = 500.0 * nx, 500.0 * nz
    setup = A.RisingBubbleSetup(ps, xc=Lx / 2, zc=Lz / 5, rc=Lx / 5)
    law = A.DryAtmosModel(setup, orientation=A.ORIENT_FLAT,
                          ref_state=A.DryAdiabaticProfile(ps, 300.0, 0.0),
                          smagorinsky=ps.C_smag, sources=A.SRC_GRAVITY,
                          boundary_conditions=(A.BC_ATMOS_DEFAULT, A.BC_ATMOS_DEFAULT),
                          param_set=ps)
    return law, grid


def ocean_spindown_setup(Nx=5, Ny=5, Nz=8, N=4, rank=0, size=1):
    """test/Ocean/HydrostaticBoussinesq/test_3D_spindown.jl:22-100: SimpleBox 1e6 x 1e6 x 400 m,
    5 x 5 x 8 elements, N = 4, periodic in x and y, boundary (1, 2) in z, c_h = 1, alpha_T =
    kappa = f = beta = 0, default viscosities; dt = 120 s, LSRK144, one day."""
    O = cm.ocean
    Lx, Ly, H = 1e6, 1e6, 400.0
    problem = O.SimpleBox(Lx, Ly, H)
    law = O.HydrostaticBoussinesqModel(problem, c_h=1.0, alpha_T=0.0, kappa_h=0.0, kappa_z=0.0,
                                       f_o=0.0, beta=0.0)
    rng = [np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1), np.linspace(-H, 0.0, Nz + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False),
                                  boundary=((0, 0), (0, 0), (1, 2)), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    return law, grid


def ocean_gyre_setup(Nx=5, Ny=5, Nz=5, N=4, rank=0, size=1, L=1e6):
    """test/Ocean/HydrostaticBoussinesq/test_ocean_gyre_short.jl with
    experiments/OceanBoxGCM/simple_box.jl: OceanGyre 1e6 x 1e6 x 1000 m, 5^3 elements, N = 4,
    c_h = sqrt(g H), every other parameter at its default, non-periodic box with boundary tags
    ((1,1),(1,1),(2,3)) (OceanBoxGCMConfiguration defaults); dt = 120 s, LSRK144, one hour."""
    O = cm.ocean
    Lx, Ly, H = L, L, 1000.0       # test_ocean_gyre_long.jl: 4e6 x 4e6 x 1000 m on 20^3 elements
    problem = O.OceanGyre(Lx, Ly, H)
    law = O.HydrostaticBoussinesqModel(problem, c_h=np.sqrt(9.81 * H))
    rng = [np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1), np.linspace(-H, 0.0, Nz + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(False, False, False),
                                  boundary=((1, 1), (1, 1), (2, 3)), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    return law, grid


def ocean_windstress_setup(Nx=5, Ny=5, Nz=5, N=4, rank=0, size=1):
    """test/Ocean/HydrostaticBoussinesq/test_windstress_short.jl (explicit run): HomogeneousBox
    1e6 x 1e6 x 400 m, 5^3 elements, no-slip walls (tag 1), free-slip bottom (tag 2), penetrable
    surface with kinematic stress (tag 3), all insulating; dt = 180 s, LSRK144, one hour."""
    O = cm.ocean
    Lx, Ly, H = 1e6, 1e6, 400.0
    BC = (O.OceanBC(O.IMPENETRABLE_NOSLIP), O.OceanBC(O.IMPENETRABLE_FREESLIP),
          O.OceanBC(O.PENETRABLE_KINEMATIC_STRESS))
    law = O.HydrostaticBoussinesqModel(O.HomogeneousBox(Lx, Ly, H, BC=BC), c_h=np.sqrt(9.81 * H))
    rng = [np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1), np.linspace(-H, 0.0, Nz + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(False, False, False),
                                  boundary=((1, 1), (1, 1), (2, 3)), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    return law, grid


def advection_sphere_setup(level=1, N=4, rank=0, size=1, problem="SolidBodyRotation", cfl=5.0):
    """test/Numerics/DGMethods/advection_diffusion/advection_sphere.jl:303-430
    (SolidBodyRotation, LSRK144 at CFL 5): cubed sphere of 2^(level-1) * 2 elements per edge,
    one element between R = 1 and R = 2, NoFlowBC on both shells, advection only, Rusanov."""
    nh = 2 ** (level - 1) * 2
    topl = M.StackedCubedSphereTopology(nh, np.linspace(1.0, 2.0, 2), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)
    prob = getattr(BL, problem)()
    law = BL.AdvectionDiffusion(3, prob, (BL.NoFlowBC(),), diffusion=False)
    dx = M.grids.min_node_distance(grid, 1)
    dt = cfl * dx / prob.u_scale
    dt = prob.finaltime / np.ceil(prob.finaltime / dt)
    return law, grid, dt


def diffusion_sphere_setup(level=1, hyper=False, N=3, rank=0, size=1):
    """diffusion_hyperdiffusion_sphere.jl:99-270: cubed sphere of 2^(level-1) * 4 elements per
    edge, N = 3, shell [1, 2] without boundary tags, diffusion_direction horizontal, central
    fluxes, LSRK54 with dt = 300 dx^4."""
    Ne = 2 ** (level - 1) * 4
    topl = M.StackedCubedSphereTopology(Ne, np.linspace(1.0, 2.0, 2), boundary=(0, 0),
                                        rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=M.equiangular_cubed_sphere_warp)
    law = BL.AdvectionDiffusion(3, BL.DiffusionSphere(hyper), (), advection=False,
                                diffusion=not hyper, hyperdiffusion=hyper)
    dx = M.grids.min_node_distance(grid)
    dt = 300 * dx ** 4
    dt = 2.0 / np.ceil(2.0 / dt)
    return law, grid, dt


def hyperdiffusion_bc_setup(level=1, N=4, rank=0, size=1):
    """hyperdiffusion_bc.jl:150-200, 300-345 (dim = 3): brick [2, 9]^3 with 2^(level-1) * 4
    elements per side, six boundary tags with mixed data of orders 0-3, H = I / 1000,
    k = (1, 1, 0), central fluxes, LSRK54 with dt = dx^4 / 100 / mu."""
    Ne = 2 ** (level - 1) * 4
    x = np.linspace(2.0, 9.0, Ne + 1)
    topl = M.StackedBrickTopology([x] * 3, periodicity=(False,) * 3,
                                  boundary=((1, 2), (3, 4), (5, 6)), connectivity="full",
                                  rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    I, H = BL.InhomogeneousBC, BL.HomogeneousBC
    bcs = ((I(0), I(2)), (I(0), I(1)), (I(3), I(1)), (I(3), I(2)), (H(3), H(1)), (H(3), H(1)))
    mu = 1 / 1000
    law = BL.AdvectionDiffusion(3, BL.HyperDiffusionBC(mu, (1, 1, 0)), bcs, advection=False,
                                diffusion=False, hyperdiffusion=True)
    dx = M.grids.min_node_distance(grid)
    dt = dx ** 4 / 100 / mu
    dt = 1.0 / np.ceil(1.0 / dt)
    return law, grid, dt


def heat_eqn_setup(level=1, direction=0, N=4, rank=0, size=1):
    """pseudo1D_heat_eqn.jl:100-150, 225-290 (dim = 3): unit cube with 2^(level-1) * 4 elements
    per side, tags (1, 2) in every direction = (Neumann data, Dirichlet data) in flux form,
    D = n n' with n along the operator's direction, LSRK144, dt = 1 / (Ne N^2)^2, t_end = 0.01."""
    n = {0: np.ones(3) / np.sqrt(3), 1: np.array([1, 1, 0]) / np.sqrt(2),
         2: np.array([0, 0, 1.0])}[direction]
    Ne = 2 ** (level - 1) * 4
    x = np.linspace(0.0, 1.0, Ne + 1)
    topl = M.StackedBrickTopology([x] * 3, periodicity=(False,) * 3, boundary=((1, 2),) * 3,
                                  connectivity="full", rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = BL.AdvectionDiffusion(3, BL.HeatEqn(n), (BL.InhomogeneousBC(1), BL.InhomogeneousBC(0)),
                                flux_bc=True, advection=False)
    dt = 1 / (Ne * N ** 2) ** 2
    nsteps = int(np.ceil(0.01 / dt))
    return law, grid, 0.01 / nsteps, nsteps


def split_explicit_setup(coupled=True, Nx=5, Ny=5, Nz=8, N=4, N_extrusion=None, rank=0, size=1,
                         rotating=False):
    """test/Ocean/SplitExplicit/hydrostatic_spindown.jl:3-140 (SplitExplicitSolver variant):
    SimpleBox 1e6 x 1e6 x 400 m, 3-D HBModel (c_h = 1, alpha_T = kappa = 0, default Coriolis
    parameters but a Fixed box, so f = -0) + 2-D ShallowWaterModel (ConstantViscosity(nu_h),
    c = 1); periodic in x and y; the barotropic model on the one-layer extrusion of the 2-D grid."""
    O = cm.ocean
    Lx, Ly, H = 1e6, 1e6, 400.0
    problem = O.SimpleBox(Lx, Ly, H, rotation=O.ROTATING if rotating else O.FIXED)
    law3 = O.HydrostaticBoussinesqModel(problem, c_h=1.0, alpha_T=0.0, kappa_h=0.0, kappa_z=0.0,
                                        coupled=coupled)
    law2 = O.ShallowWaterModel(problem, law3.nu_h, advection=False, coupled=coupled, c=1.0)
    x, y = np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1)
    topl = M.StackedBrickTopology([x, y, np.linspace(-H, 0.0, Nz + 1)],
                                  periodicity=(True, True, False), boundary=((0, 0), (0, 0), (1, 2)),
                                  rank=rank, size=size)
    grid3 = M.DiscontinuousSpectralElementGrid(topl, N)
    grid2 = O.extruded_barotropic_grid(x, y, N, N_extrusion=N_extrusion, rank=rank, size=size)
    return law3, grid3, law2, grid2


def split_explicit_schedule(dt_slow, tout=3 * 3600.0, timeend=86400.0):
    """run_split_explicit (test/Ocean/SplitExplicit/hydrostatic_spindown.jl:60-75): the slow
    step is shortened so that an integer number of steps reaches the output interval."""
    nout = int(np.ceil(tout / dt_slow))
    dt = tout / nout
    return dt, int(round(timeend / dt))


def statecheck(a):
    """``scstats`` (src/Diagnostics/Debug/StateCheck.jl:231-283)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    m = a.mean()
    return a.min(), a.max(), m, np.sqrt(((a - m) ** 2).sum() / (a.size - 1))


def split_explicit_fields(Q3, A3, Q2, A2, grid2):
    """The twenty rows of the reference table; the 2-D arrays are read on the k = 0 plane of the
    one-layer extrusion (the reference's 2-D grid has exactly those nodes)."""
    Nqh = grid2.Nq[0] * grid2.Nq[1]
    q0 = np.asarray(Q2).reshape(grid2.nelem, Q2.shape[1], grid2.Nq[2], Nqh)[:grid2.nreal, :, 0, :]
    a0 = np.asarray(A2).reshape(grid2.nelem, A2.shape[1], grid2.Nq[2], Nqh)[:grid2.nreal, :, 0, :]
    f = {}
    for i, n in enumerate(("u[1]", "u[2]", "η", "θ")):
        f[("3D state", n)] = Q3[:, i]
    for i, n in enumerate(("y", "w", "pkin", "wz0", "uᵈ[1]", "uᵈ[2]", "ΔGᵘ[1]", "ΔGᵘ[2]")):
        f[("3D aux", n)] = A3[:, i]
    for i, n in enumerate(("η", "U[1]", "U[2]")):
        f[("2D state", n)] = q0[:, i]
    for i, n in enumerate(("y", "Gᵁ[1]", "Gᵁ[2]", "Δu[1]", "Δu[2]")):
        f[("2D aux", n)] = a0[:, i]
    return f


def check_split_explicit_table(table, parr, fields, slack=2.0):
    """Every statistic the reference checks (precision > 0 in ``parr``), to ``slack`` units of
    its stated digit; exact zeros must be exact.  Returns the worst relative deviation."""
    worst = 0.0
    for row, prow in zip(table, parr):
        key = (row[0], row[1])
        assert key == (prow[0], prow[1])
        got = statecheck(fields[key])
        for j in range(4):
            p = int(prow[2 + j])
            if p == 0:
                continue
            ref = row[2 + j]
            if ref == 0:
                assert got[j] == 0, (key, j, got[j])
                continue
            rel = abs(got[j] - ref) / abs(ref)
            worst = max(worst, rel * 10.0 ** p)
            assert rel <= slack * 10.0 ** (-p), (key, j, got[j], ref, rel)
    return worst


def scdocheck_match(cur, ref, pcmp):
    """The acceptance rule of the reference's ``scdocheck`` (src/Diagnostics/Debug/StateCheck.jl:
    404-452), character for character: both numbers printed with ``%28.20e``; equal exponents,
    then the characters 2 .. pcmp + 4 (sign, leading digit, point, digits) compared left to right;
    failing that, ``round(log10(relative difference)) < -pcmp``.  Returns the number of matching
    characters (>= pcmp passes)."""
    import math
    cv, rv = "%28.20e" % cur, "%28.20e" % ref
    nmatch = 0
    if cv[24:28] == rv[24:28]:
        for a, b in zip(cv[1:pcmp + 4], rv[1:pcmp + 4]):
            if a != b:
                break
            nmatch += 1
    if nmatch < pcmp and cur != ref:
        e = round(math.log10(abs((ref - cur) / ref))) if ref != 0 else round(math.log10(abs(ref - cur)))
        if e < -pcmp:
            nmatch = int(-e)
    return nmatch


def check_statecheck_table(table, parr, fields, relaxed=None, report=None):
    """Every row of a reference StateCheck table under the reference's own rule
    (:func:`scdocheck_match`); ``relaxed[(array, field)]`` lowers the required digits of a row
    (documented where used).  Returns (worst relative deviation in units of the stated digit,
    fewest matching characters beyond the requirement); ``report`` (a list) receives one line per
    statistic."""
    worst, margin, bad = 0.0, 99, []
    for row, prow in zip(table, parr):
        key = (row[0], row[1])
        assert key == (prow[0], prow[1])
        got = statecheck(fields[key])
        for j in range(4):
            p = int(prow[2 + j])
            if p == 0:
                continue
            if relaxed and key in relaxed:
                p = min(p, relaxed[key])
            ref = row[2 + j]
            n = scdocheck_match(got[j], ref, p)
            rel = abs(got[j] - ref) / abs(ref) if ref != 0 else abs(got[j])
            if report is not None:
                report.append("%-10s %-8s %-4s digits %2d of %2d  rel %.1e" % (
                    key[0], key[1], ("min", "max", "mean", "std")[j], n, p, rel))
            if n < p:
                bad.append((key, ("min", "max", "mean", "std")[j], got[j], ref, n, p))
            margin = min(margin, n - p)
            worst = max(worst, rel * 10.0 ** p)
    assert not bad, bad
    return worst, margin


def mms_atmos_setup(level=1, N=4):
    """test/Numerics/DGMethods/compressible_Navier_Stokes/mms_bc_atmos.jl, dim = 3: unit cube,
    (4 * 2^(level-1))^3 elements, warped (:252-262), every face InitStateBC; dry AtmosModel with
    ConstantDynamicViscosity(1/100, WithDivergence()), NoReferenceState, NoOrientation,
    T_0 = 0, total_specific_enthalpy == 0, MMSSource{3}; dt = 5e-3 / Ne rounded to divide 1.
    (The reference builds a BrickTopology; the stacked topology holds the same elements in another
    order, which the error norm does not see.)"""
    A = cm.atmos
    ps = A.PlanetParameters()
    ps.T_0 = 0.0
    Ne = 4 * 2 ** (level - 1)
    r = np.linspace(0.0, 1.0, Ne + 1)
    topl = M.StackedBrickTopology([r, r, r], periodicity=(False, False, False),
                                  boundary=((1, 1), (1, 1), (1, 1)))

    def warp(x1, x2, x3):
        return (x1 + (x1 - 1 / 2) * np.cos(2 * np.pi * x2 * x3) / 4,
                x2 + np.exp(np.sin(2 * np.pi * (x1 * x2 + x3))) / 20,
                x3 + x1 / 4 + x2 ** 2 / 2 + np.sin(x1 * x2 * x3))

    grid = M.DiscontinuousSpectralElementGrid(topl, N, meshwarp=warp)
    law = A.DryAtmosModel(A.MMSSetup(ps), orientation=A.ORIENT_NONE, ref_state=None,
                          viscosity=1 / 100, dynamic_viscosity=True, with_divergence=True,
                          zero_enthalpy=True, sources=A.SRC_MMS,
                          boundary_conditions=(A.BC_INIT_STATE_MMS,), param_set=ps)
    nsteps = int(np.ceil(1.0 / (5e-3 / Ne)))
    return law, grid, 1.0 / nsteps, nsteps


def density_current_setup(Ne=(100, 2, 50), N=4):
    """test/Numerics/DGMethods/compressible_Navier_Stokes/density_current_model.jl:41-175:
    12.8 km x 400 m x 6.4 km, 100 x 2 x 50 elements, periodic in y, default AtmosBC elsewhere,
    EquilMoist (q_tot = 0), AnisoMinDiss(1), HydrostaticState(DryAdiabaticProfile(param_set)),
    Gravity, Rusanov; dt = 0.01 s, ten LSRK54 steps."""
    A, MO = cm.atmos, cm.moist
    ps = MO.MoistParameters()
    rng = [np.linspace(0.0, 12800.0, Ne[0] + 1), np.linspace(0.0, 400.0, Ne[1] + 1),
           np.linspace(0.0, 6400.0, Ne[2] + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(False, True, False),
                                  boundary=((1, 1), (0, 0), (1, 1)))
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = MO.MoistAtmosModel(MO.DensityCurrentSetup(ps), A.DryAdiabaticProfile(ps, 290.0, 220.0),
                             closure=MO.CLOSURE_ANISO_MIN_DISS, coefficient=1.0,
                             boundary_conditions=(A.BC_ATMOS_DEFAULT,), param_set=ps)
    return law, grid, 0.01, 10


def bomex_setup(nx=4, ny=4, nz=8, N=4, rank=0, size=1, zmax=3000.0, L=None):
    """experiments/AtmosLES/bomex_les.jl through AtmosLESConfiguration: periodic in x and y,
    boundary (1, 2) in z, 3 km deep; the reference uses 6.4 km x 6.4 km at (100, 100, 40) m
    resolution, the tests a reduced box with the same element aspect."""
    MO = cm.moist
    L = L if L is not None else 400.0 * nx
    rng = [np.linspace(0.0, L, nx + 1), np.linspace(0.0, L * ny / nx, ny + 1),
           np.linspace(0.0, zmax, nz + 1)]
    topl = M.StackedBrickTopology(rng, periodicity=(True, True, False),
                                  boundary=((0, 0), (0, 0), (1, 2)), rank=rank, size=size)
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    return MO.bomex_model(zmax), grid


def simple_box_2dt_setup(Nx=20, Ny=20, Nz=20, N=4, N_extrusion=1, rank=0, size=1):
    """test/Ocean/SplitExplicit/simple_box_2dt.jl:478-517: 4e6 m x 4e6 m x 1000 m box, wind
    stress 0.2 Pa, surface relaxation 20 m / day towards 10 (1 - y / Ly), no-slip coasts and
    floor (tags 1, 2), stress + forcing surface (tag 3), c_h = 1, grav from CLIMAParameters,
    add_fast_substeps = 2; slow step 5400 s, fast step 240 s, five days."""
    O1, O = cm.ocean01, cm.ocean
    Lx, Ly, H = 4e6, 4e6, 1000.0
    problem = O1.SimpleBox01(Lx, Ly, H, tau_o=2e-1, lambda_r=20 / 86400, theta_E=10.0)
    model = O1.OceanModel01(problem, grav=9.81, c_h=1.0, add_fast_substeps=2)
    baro = O1.BarotropicModel01(model)
    x, y, z = np.linspace(0.0, Lx, Nx + 1), np.linspace(0.0, Ly, Ny + 1), np.linspace(-H, 0.0, Nz + 1)
    topl = M.StackedBrickTopology([x, y, z], periodicity=(False, False, False),
                                  boundary=((1, 1), (1, 1), (2, 3)), rank=rank, size=size)
    grid3 = M.DiscontinuousSpectralElementGrid(topl, N)
    grid2 = O.extruded_barotropic_grid(x, y, N, periodicity=(False, False),
                                       boundary=((1, 1), (1, 1)), N_extrusion=N_extrusion,
                                       rank=rank, size=size)
    return model, grid3, baro, grid2


def simple_box_2dt_fields(Q3, A3, Q2, A2, grid2):
    """The 28 rows of test/Ocean/refvals/simple_box_2dt_refvals.jl; 2-D arrays on the k = 0
    plane of the one-layer extrusion."""
    O1 = cm.ocean01
    Nqh = grid2.Nq[0] * grid2.Nq[1]
    q0 = np.asarray(Q2).reshape(grid2.nelem, Q2.shape[1], grid2.Nq[2], Nqh)[:grid2.nreal, :, 0, :]
    a0 = np.asarray(A2).reshape(grid2.nelem, A2.shape[1], grid2.Nq[2], Nqh)[:grid2.nreal, :, 0, :]
    f = {}
    for i, n in enumerate(O1.STATE_NAMES_3D):
        f[("oce Q_3D", n)] = Q3[:, i]
    for i, n in enumerate(O1.AUX_NAMES_3D):
        f[("oce aux", n)] = A3[:, i]
    for i, n in enumerate(O1.STATE_NAMES_2D):
        f[("baro Q_2D", n)] = q0[:, i]
    for i, n in enumerate(O1.AUX_NAMES_2D):
        f[("baro aux", n)] = a0[:, i]
    return f


def isentropic_vortex_moist_setup(level=1, N=4):
    """test/Numerics/DGMethods/Euler/isentropicvortex.jl:308-370 with ``moisture = EquilMoist()``
    (the RoeNumericalFluxMoist rows): dims = 3, NoReferenceState, NoOrientation,
    ConstantDynamicViscosity(0), periodic BrickTopology, rho q_tot = 0."""
    MO = cm.moist
    ps = MO.MoistParameters()
    setup = MO.IsentropicVortexMoistSetup(ps)
    L = setup.domain_halflength
    numelems = (2 ** (level - 1) * 5, 2 ** (level - 1) * 5, 1)
    rng = [np.linspace(-L, L, n + 1) for n in numelems]
    topl = M.BrickTopology(rng, periodicity=(True,) * 3, connectivity="face")
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = MO.MoistAtmosModel(setup, None, closure=MO.CLOSURE_CONSTANT, coefficient=0.0,
                             kinematic=False, subtract_off=False, sources=0, boundary_conditions=(),
                             param_set=ps, no_orientation=True)
    timeend = 2 * L / 10 / setup.translation_speed
    elementsize = min(2 * L / n for n in numelems)
    cs = np.sqrt(ps.cp_d / ps.cv_d * ps.R_d * setup.T_inf)
    dt = elementsize / cs / N ** 2
    nsteps = int(np.ceil(timeend / dt))
    return law, grid, timeend / nsteps, timeend, nsteps


# ---- the reference's dim = 2 problems on the 3-D kernels -----------------------------------
# A 2-D grid (xi1 horizontal, xi2 vertical) is the y-invariant slice of a 3-D one: one periodic
# element across y, fields constant in y, 2-D vectors (a, b) embedded as (a, 0, b).  The xi2
# derivative and the y-face terms then vanish (to rounding), what remains is the 2-D operator,
# and mass-weighted norms carry the factor sqrt(Ly).
DIM2_N = {0: np.array([1.0, 0.0, 1.0]) / np.sqrt(2), 1: np.array([1.0, 0.0, 0.0]),
          2: np.array([0.0, 0.0, 1.0])}


def pseudo1d_dim2_setup(Ne=4, N=4, direction=0, flux_bc=False):
    """pseudo1D_advection_diffusion.jl:293-368 with dim = 2 (n = (1,1)/sqrt 2, (1,0), (0,1))."""
    x = np.linspace(-1, 1, Ne + 1)
    Ly = 2.0 / Ne
    topl = M.StackedBrickTopology([x, np.array([0.0, Ly]), x],
                                  boundary=((1, 2), (0, 0), (1, 2)),
                                  periodicity=(False, True, False), connectivity="full")
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = BL.AdvectionDiffusion(3, BL.Pseudo1D(DIM2_N[direction], 1.0, 1 / 100, -1 / 2, 1 / 10),
                                (BL.InhomogeneousBC(0), BL.InhomogeneousBC(1)), flux_bc=flux_bc)
    dt = (1.0 / 4) / (Ne * N ** 2)
    dt = 1.0 / np.ceil(1.0 / dt)
    return law, grid, dt, np.sqrt(Ly)


class _HyperDiffusionDim2(BL.ConstantHyperDiffusion):
    """ConstantHyperDiffusion{2, dir} (periodic_3D_hyperdiffusion.jl:40-63): k = (1, 2) and
    D[1:2, 1:2], embedded as k = (1, 0, 2) and the (x, z) block of a 3 x 3 tensor."""

    def __init__(self, direction, D):
        D = np.asarray(D, dtype=np.float64)
        D3 = np.zeros((3, 3))
        for a, i in enumerate((0, 2)):
            for b, j in enumerate((0, 2)):
                D3[i, j] = D[a, b]
        super().__init__(3, direction, D3)
        self.D2 = D[:2, :2].copy()

    def _c(self):
        k = np.array([1.0, 2.0])
        kD = (k[:, None] * k[None, :]) * self.D2
        if self.direction == BL.EveryDirection:
            return (k[0] * k[0] + k[1] * k[1]) * (kD[0, 0] + kD[1, 0] + kD[0, 1] + kD[1, 1])
        if self.direction == BL.HorizontalDirection:
            return k[0] * k[0] * kD[0, 0]
        return k[1] ** 2 * kD[1, 1]

    def initial_condition(self, coord, t):
        return np.sin(1.0 * coord[0] + 2.0 * coord[2]) * np.exp(-self._c() * t)


def periodic_hyperdiffusion_dim2_setup(Ne=4, N=4, direction=0):
    """periodic_3D_hyperdiffusion.jl:107-322 with dim = 2."""
    D = np.array([[9, 3, 5], [3, 7, 4], [5, 4, 10]], dtype=np.float64) / 50 / 100
    x = np.linspace(0.0, 2 * np.pi, Ne + 1)
    Ly = 2 * np.pi / Ne
    topl = M.StackedBrickTopology([x, np.array([0.0, Ly]), x], periodicity=(True,) * 3,
                                  connectivity="full")
    grid = M.DiscontinuousSpectralElementGrid(topl, N)
    law = BL.AdvectionDiffusion(3, _HyperDiffusionDim2(direction, D), (),
                                advection=False, diffusion=False, hyperdiffusion=True)
    dx = M.grids.min_node_distance(grid)
    dt = dx ** 4 / 25 / D.sum()
    dt = 1.0 / np.ceil(1.0 / dt)
    return law, grid, dt, np.sqrt(Ly)


# ---- the moist law away from the warm branch ----------------------------------------------------
def moist_converged_law(closure=1, **kw):
    """The moist LES law of the cloudy-bubble tests with a converged saturation adjustment
    (maxiter 40, tolerance 1e-11 K); the state comes from the caller, not from the law."""
    A, MO = cm.atmos, cm.moist
    ps = MO.MoistParameters()
    kw.setdefault("coefficient", {0: 75.0, 1: ps.C_smag, 2: 1.0}[closure])
    return MO.MoistAtmosModel(None, A.DryAdiabaticProfile(ps, 300.0, 0.0), closure=closure, param_set=ps,
                              maxiter=40, tolerance=1e-11, **kw)


def periodic_brick_grid(L=1500.0, N=4):
    """The grid of ``isentropic_vortex_moist_setup(1)`` (periodic BrickTopology, 5 x 5 x 1 elements,
    face connectivity) stretched to ``[0, L]^3``, so that a law with an orientation has a potential
    of thousands of J/kg across it."""
    rng = [np.linspace(0.0, L, n + 1) for n in (5, 5, 1)]
    topl = M.BrickTopology(rng, periodicity=(True,) * 3, connectivity="face")
    return M.DiscontinuousSpectralElementGrid(topl, N)


def tile_moist_phase_cases(grid, aux, cases, seed=0):
    """One case of tests/golden/moist_phase_cases.npz per node, tiled over the grid: ``rho`` and
    ``q_tot`` as stored, ``rho e = rho (e_int + Phi + |u|^2 / 2)`` with ``Phi`` from ``aux`` and random
    winds of a few m/s.  Returns ``(Q, index of the case at every node)``."""
    n = len(cases["rho"])
    idx = (np.arange(grid.nelem * grid.Np) % n).reshape(grid.nelem, grid.Np)
    rng = np.random.default_rng(seed)
    u = 3.0 * rng.standard_normal((grid.nelem, 3, grid.Np))
    rho = cases["rho"][idx]
    Q = np.zeros((grid.nelem, 6, grid.Np))
    Q[:, 0] = rho
    Q[:, 1:4] = rho[:, None, :] * u
    Q[:, 4] = rho * (cases["e_int"][idx] + aux[:, 3] + (u * u).sum(axis=1) / 2)
    Q[:, 5] = rho * cases["q_tot"][idx]
    return Q, idx


def cold_cloudy_state(law, grid, aux, jet=0.0):
    """A smooth state that crosses every phase regime of the equilibrium thermodynamics: the
    equilibrium temperature falls from about 295 K at the bottom of the box to 221 K at its top with
    a horizontal sine of 3 K, the supersaturation ``s = 0.15 sin(...)`` changes sign across the box
    (``q_tot = q_vs(T*, rho) (1 + s)``: cloudy where ``s > 0``, with liquid, both phases or ice by
    temperature; unsaturated where ``s < 0``), the density is smooth and the winds are of a few m/s.
    ``jet`` (m/s) adds a zonal jet at mid-height, in the mixed-phase layer, strongest where ``s`` is
    largest: a maximum over the nodes of ``|u| + c`` then sits on a mixed-phase node instead of on
    the warmest one.  Not a reference configuration."""
    ps = law.ps
    unit = []
    for d in range(3):
        lo, hi = aux[:, d].min(), aux[:, d].max()
        unit.append((aux[:, d] - lo) / (hi - lo))
    xi, eta, zeta = unit
    T = 295.0 - 74.0 * zeta + 3.0 * np.sin(2 * np.pi * xi) * np.cos(2 * np.pi * eta)
    s = 0.15 * np.sin(2 * np.pi * (xi + eta) + 3 * np.pi * zeta)
    rho = 1.1 - 0.5 * zeta + 0.03 * np.cos(2 * np.pi * xi)
    lam = np.clip((T - ps.T_icenuc) / (ps.T_freeze - ps.T_icenuc), 0.0, 1.0)
    LH_0 = lam * ps.LH_v0 + (1 - lam) * ps.LH_s0
    dcp = lam * (ps.cp_v - ps.cp_l) + (1 - lam) * (ps.cp_v - ps.cp_i)
    p_vs = ps.press_triple * (T / ps.T_triple) ** (dcp / ps.R_v) * np.exp(
        (LH_0 - dcp * ps.T_0) / ps.R_v * (1 / ps.T_triple - 1 / T))
    q_vs = p_vs / (rho * ps.R_v * T)
    q_tot = q_vs * (1 + s)
    q_c = np.maximum(q_tot - q_vs, 0.0)
    e_int = ps.internal_energy(T, q_tot, lam * q_c, (1 - lam) * q_c)
    u = [3.0 * np.sin(2 * np.pi * xi) * np.cos(2 * np.pi * eta) + jet * np.sin(np.pi * zeta) ** 2 * (1 + s),
         2.0 * np.cos(2 * np.pi * xi),
         1.5 * np.sin(2 * np.pi * (xi + eta)) * np.sin(np.pi * zeta)]
    Q = np.zeros((grid.nelem, 6, grid.Np))
    Q[:, 0] = rho
    for d in range(3):
        Q[:, 1 + d] = rho * u[d]
    Q[:, 4] = rho * (e_int + aux[:, law.off_phi] + (u[0] ** 2 + u[1] ** 2 + u[2] ** 2) / 2)
    Q[:, 5] = rho * q_tot
    return Q


def phase_census(aux):
    """Node counts of the refreshed moisture block ``aux[:, 15:19]``: ice only, mixed (liquid and
    ice both above 1e-6), warm cloudy, unsaturated."""
    T, ql, qi = aux[:, 15], aux[:, 17], aux[:, 18]
    return dict(ice=int(((ql == 0) & (qi > 0)).sum()), mixed=int(((ql > 1e-6) & (qi > 1e-6)).sum()),
                warm=int(((ql > 0) & (qi == 0)).sum()), unsaturated=int(((ql == 0) & (qi == 0)).sum()),
                T_min=float(T.min()), T_max=float(T.max()))


OBSERVED = {}


def observe(name, value):
    """Records the largest value seen under ``name`` (written to gpurun_out/observed_maxima.json
    at the end of the session, tests/conftest.py) and returns it: for tolerances looser than the
    north star's 1e-12, so that what the device actually reaches stands next to the bound."""
    v = float(value)
    if not (OBSERVED.get(name, -1.0) >= v):
        OBSERVED[name] = v
    return value
