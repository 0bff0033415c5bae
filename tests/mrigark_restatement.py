"""A NumPy restatement of the two MRI-GARK ``dostep!``s (MultirateInfinitesimalGARKExplicit.jl,
MultirateInfinitesimalGARKDecoupledImplicit.jl) with a low-storage 2N fast method whose stages
carry the MRI forcing (``lsrk_mri_update!``, LowStorageRungeKuttaMethod.jl:174-225), in the
operation order of the device step (csrc/multirate.hip).  Shared by tests/test_mrigark_host.py
(the two-rate ODE) and tests/test_gpu_mrigark.py (oracle DG operators)."""


def fast_solve(Q, dQ, fast_inc, tableau, fast_dt, ts, timeend, dts, gammas, Rs, rv=slice(None)):
    """``updatetime!(fast, ts); solve!(Q, fast, mriparam; timeend)`` with adjustfinalstep:
    ``fast_inc(dQ, Q, t)`` adds the fast tendency to ``dQ``; ``gammas[k][j]`` the coupling
    coefficients of ``Rs[j]``."""
    RKA, RKB, RKC = tableau
    n = len(RKA)
    time = ts
    while time < timeend:
        dt = fast_dt
        final = False
        if time + dt > timeend:
            dt = timeend - time
            final = True
        for s in range(n):
            stage_time = time + RKC[s] * dt
            fast_inc(dQ, Q, stage_time)
            tau = (stage_time - ts) / dts
            dq = dQ[rv].copy()
            for j in range(len(Rs)):
                sc = gammas[-1][j]
                for k in range(len(gammas) - 2, -1, -1):
                    sc = sc * tau + gammas[k][j]
                dq = dq + sc * Rs[j][rv]
            Q[rv] = Q[rv] + (RKB[s] * dt) * dq
            dQ[rv] = RKA[(s + 1) % n] * dq
        time = timeend if final else time + dt


def explicit_step(Q, t, dt, G, dc, slow, fast_inc, dQ, tableau, fast_dt, Rs, rv=slice(None)):
    """``dostep!(Q, ::MRIGARKExplicit, p, t)``: ``G`` the scaled ``Γ_k ./ Δc``, ``slow(R, Q, t)``
    the slow tendency (increment = false)."""
    ts = t
    for s in range(len(dc)):
        dts = dc[s] * dt
        slow(Rs[s], Q, ts)
        gam = [[G[k][s][j] for j in range(s + 1)] for k in range(len(G))]
        fast_solve(Q, dQ, fast_inc, tableau, fast_dt, ts, ts + dts, dts, gam, Rs[:s + 1], rv)
        ts += dts


def implicit_step(Q, t, dt, G, dc, slow, besolve, fast_inc, dQ, tableau, fast_dt, Rs, Qhat,
                  rv=slice(None)):
    """``dostep!(Q, ::MRIGARKDecoupledImplicit, p, t)``: ``G`` the raw ``Γ_k``,
    ``besolve(Q, Qhat, alpha, t)`` solves ``Q = Qhat + alpha slow(Q, t)``."""
    ts = t
    for s in range(len(dc)):
        dts = dc[s] * dt
        stage_end = ts + dts
        slow(Rs[s], Q, ts)
        gam = [[G[k][2 * s][j] / dc[s] for j in range(s + 1)] for k in range(len(G))]
        fast_solve(Q, dQ, fast_inc, tableau, fast_dt, ts, stage_end, dts, gam, Rs[:s + 1], rv)
        qh = Q[rv].copy()
        for j in range(s + 1):
            sc = dt * G[0][2 * s + 1][j]
            for k in range(1, len(G)):
                sc += dt * G[k][2 * s + 1][j] / (k + 1)
            qh = qh + sc * Rs[j][rv]
        Qhat[rv] = qh
        besolve(Q, Qhat, dt * G[0][2 * s + 1][s + 1], stage_end)
        ts += dts
