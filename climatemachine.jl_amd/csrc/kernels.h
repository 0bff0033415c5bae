// Hand-written gfx950 kernels of the DG hot path.  One workgroup per element (the tendency pass
// of elements above N = 4 takes two, see TendencyShape):
//   phase 1  thread = volume node: pointwise physics, contravariant fluxes / gradient
//            arguments staged in LDS;
//   phase 2  thread = volume node: (N+1)-point contractions with D out of LDS, result
//            into an LDS accumulator;
//   phase 3  thread = face node (6 faces x Nfp tasks at once): numerical / boundary
//            fluxes, lifted into the LDS accumulator one opposite-face pair at a time
//            (race free, reference order);
//   phase 4  thread = volume node: one coalesced store per output field (for the
//            tendency kernel with the LSRK update fused in).
// Each kernel replaces a *group* of reference kernels (horizontal + vertical volume
// kernel and the per-direction interface launches) of
// src/Numerics/DGMethods/DGModel_kernels.jl; the accumulation order of the reference
// is kept term by term (see DESIGN.md "summation order").
#pragma once
#include "kernels_common.h"
#include "kernels_gradients.h"
#include "kernels_nodal.h"
#include "kernels_tendency.h"
