// Test-only host build of the host side of iso_shared_cut_kernel's argument block (ssde_device.hpp: HeadArgs, head_args_fill,
// head_ns_min, head_lead_groups): plain host code of a header that also declares kernels' arguments, so the HIP runtime's header is on
// the include path and nothing of the runtime is linked or called.  tests/test_head_prologue_host.py.
#include <cstring>

#include "../../smoothsde_amd/csrc/ssde_device.hpp"

using namespace ssde;

extern "C" {

void hostsim_head_ns_min(const int32_t* lane_ns, int n_groups, int32_t* out) { head_ns_min(lane_ns, n_groups, out); }
int hostsim_head_lead_groups(const int32_t* glen, int n_groups) { return head_lead_groups(glen, n_groups); }
int hostsim_head_args_bytes() { return (int)sizeof(HeadArgs); }
int hostsim_iso_args_bytes() { return (int)sizeof(IsoArgs); }

// An IsoArgs whose every byte differs from its neighbours (so no two fields of one type hold the same value), through head_args_fill;
// returns a bit per field that is NOT the IsoArgs' (0: every field arrived), the fields in the order of the struct.
unsigned long long hostsim_head_args_check(int gain_rows, int lead_n, long long lead_stride, int with_ns_min) {
    IsoArgs a;
    unsigned char* b = (unsigned char*)&a;
    for (size_t i = 0; i < sizeof(IsoArgs); i++) b[i] = (unsigned char)(1 + (i * 131 + i / 251) % 255);
    static const int32_t some[1] = {7};
    HeadLead lead = {with_ns_min ? some : nullptr, lead_stride, lead_n};
    HeadArgs o;
    memset(&o, 0, sizeof o);
    head_args_fill(o, a, lead, gain_rows);
    unsigned long long bad = 0;
    int k = 0;
    auto chk = [&](bool same) { if (!same) bad |= 1ull << k; k++; };
    chk(memcmp(&o.tv, &a.tv, sizeof(TileView)) == 0);
    chk(o.ns_min == lead.ns_min);
    chk(o.lead_stride == lead_stride);
    chk(o.lead_n == lead_n);
    chk(o.n_chunks == a.n_chunks); chk(o.window == a.window); chk(o.t0 == a.t0); chk(o.t0_delta == a.t0_delta);
    chk(o.gain_last == a.gain_last); chk(o.gain_rows == gain_rows); chk(o.stream_nt == a.stream_nt);
    chk(memcmp(&o.gain_stat0, &a.gain_stat[0], 8) == 0);
    chk(o.gain == a.gain);
    chk(memcmp(o.mu, a.mu, sizeof o.mu) == 0);
    chk(memcmp(&o.ctr, &a.ctr, sizeof(CtcrwTrans)) == 0);
    chk(memcmp(o.statc, a.statc, sizeof o.statc) == 0);
    chk(o.mbx == a.mbx); chk(o.mbx_seq == a.mbx_seq); chk(o.partials == a.partials); chk(o.chk == a.chk); chk(o.chk_out == a.chk_out);
    chk(o.wave_clock == a.wave_clock);
    return bad;
}
int hostsim_head_statc() { return HEAD_STATC; }

}
