// warm_probe_emu.cpp — the CPU execution of the device source (tests/wave_emu/wave_emu.cpp, unchanged) once more, with the two
// warm-start hooks of hdsm_wave_gib.h defined: it counts what WaveGIB::warm_start does with the rows of a guess and holds the
// multiplier of every accepted row, as the probe forms it, against the full evaluation t = U^T v, lambda = U t on the same set.
// TEST INFRASTRUCTURE ONLY (tests/test_warm_probe.py).
namespace wprobe {
void note(int event, int thread);
void check(double probe, double full);
}  // namespace wprobe
#define HDSM_WARM_AUDIT(event) wprobe::note((int)(event), (int)HDSM_TX);
#define HDSM_WARM_AUDIT_CHECK(probe, full) wprobe::check((probe), (full));

#include "../wave_emu/wave_emu.cpp"

namespace wprobe {
long g_count[hdsm::WARM_EV_COUNT];
long g_checked = 0;
double g_worst = 0.0;  // largest |probe - full| / (1 + |full|) over the accepted rows
// (every lane of wave 0 passes a wave-uniform event: thread 0 counts it; a row of an input or state box is noted by the lane that holds it)
void note(int event, int thread) {
  if (event == hdsm::WARM_EV_BOX_ROW || thread == 0) ++g_count[event];
}
void check(double probe, double full) {
  const double e = fabs(probe - full) / (1.0 + fabs(full));
  ++g_checked;
  if (!(e <= g_worst)) g_worst = e;  // (a NaN stays)
}
}  // namespace wprobe

// out[0 .. WARM_EV_COUNT): the events since the last reset (hdsm::WarmEvent), out[WARM_EV_COUNT] = accepted rows checked;
// *worst = their largest relative multiplier difference. reset != 0 clears everything afterwards.
extern "C" int wave_warm_audit(long* out, double* worst, int reset) {
  for (int k = 0; k < hdsm::WARM_EV_COUNT; ++k) out[k] = wprobe::g_count[k];
  out[hdsm::WARM_EV_COUNT] = wprobe::g_checked;
  *worst = wprobe::g_worst;
  if (reset) {
    for (int k = 0; k < hdsm::WARM_EV_COUNT; ++k) wprobe::g_count[k] = 0;
    wprobe::g_checked = 0, wprobe::g_worst = 0.0;
  }
  return hdsm::WARM_EV_COUNT;
}
