// AtmosLESDefault diagnostics (cmdg_les_*): the level reductions, their finishing arithmetic and the
// ABI entries live in diagnostics.hip; the nodal pass needs the law and is launched by EngineT
// (engine.h, kernels.h k_les_nodal).  Like the reductions, the per-handle state is kept in a table of
// diagnostics.hip: nothing here changes the layout of EngineBase.
#pragma once

namespace cmdg {
struct EngineBase;
// frees the diagnostics state of an engine that is being destroyed (its device current)
void les_release(EngineBase *e);
}  // namespace cmdg
