// Host instantiation of csrc/reservoir_da.hpp for tests/test_reservoir_da_handover.py: the hand-over between two windows or two
// days of a stream, and the two data-assimilation steps, as the kernels compile them.  Build: g++ -O2 -ffp-contract=off -shared.
#include "reservoir_da.hpp"

extern "C" {
// st: update_time prev_persisted persistence_index persistence_update_time; idx: timeseries_idx (both in place)
void da_handover(int kind, float *st, int *idx, float t_end)
{
    trmc::ResDaState s{st[0], st[1], st[2], st[3], *idx};
    s = trmc::reservoir_da_handover(kind, s, t_end);
    st[0] = s.update_time;
    st[1] = s.prev_persisted;
    st[2] = s.persistence_index;
    st[3] = s.persistence_update_time;
    *idx = s.timeseries_idx;
}
// fin [12], fout [6]: the layouts of trmc_reservoir_da_steps (include/trmc.h)
void da_hybrid_step(const float *obs, const float *time, int ncol, const float *f, float *o)
{
    const trmc::HybridIn in{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9], f[10], f[11]};
    const trmc::HybridOut r = trmc::hybrid_da_step(obs, time, ncol, in);
    o[0] = r.outflow;
    o[1] = r.persisted_outflow;
    o[2] = r.water_elevation;
    o[3] = r.update_time;
    o[4] = r.persistence_index;
    o[5] = r.persistence_update_time;
}
}
