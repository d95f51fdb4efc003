// ssde_reduce_host.hpp -- the final sums of an evaluation formed on the host, in reduce_slot's order (ssde_device.hpp), from the records
// the workgroups of iso_shared_wg_kernel (k_iso_shared.inc) store into the host's mailbox: per track group, `n_windows` windows of
// `nacc` wave sums and the group's hand-over check.  Plain double additions in the fixed order of the device's reduction -- entries
// i = c G + g (window-major) and the by-value lag entry after the last one; 256 virtual threads that stride by 1024 and add
// (v0 + v1) + (v2 + v3); the 128 .. 1 tree; then add[] and map[] -- so the result is bitwise what iso_finalize_kernel and
// fused_finalize_wave give.  Host code only, no HIP type: the engine calls it after its spin on the mailbox, tests/test_head_finish_host.py
// drives the exported ssde_reduce_host against a numpy mirror.
#ifndef SSDE_REDUCE_HOST_HPP
#define SSDE_REDUCE_HOST_HPP
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace ssde_engine {

struct ReduceHostArgs {
    const double* sums;            // sums[g * group_stride + c * nacc + k]
    int64_t group_stride;
    const double* chk;             // chk[g * chk_stride]: the group's largest relative hand-over disagreement
    int64_t chk_stride;
    int n_groups, n_windows, nacc;
    const double* lag_acc;         // the bulk's forms, `nacc` accumulators: the entry after the last one; NULL: none
    double lag_chk;                // ... and their check, folded into out[n_out] by max
    const double* add;             // [4] data-independent terms, added to out[add_slot[i]] (slot < 0: unused)
    const int16_t* add_slot;
    const int16_t* map;            // [nacc - 1] accumulator k >= 1 -> output slot, or < 0
    int n_out;                     // out: n_out sums, then the check
};

// a non-negative double as the word the checks are compared by (not a number: infinity) -- lag_chk_bits of ssde_device.hpp
inline uint64_t check_bits(double w) {
    const double v = w == w ? std::fabs(w) : std::numeric_limits<double>::infinity();
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
}

// scratch: kept by the caller between calls (no allocation per evaluation)
inline void reduce_host(const ReduceHostArgs& a, double* out, std::vector<double>& scratch) {
    const int G = a.n_groups, total = a.n_windows * G, total_x = total + (a.lag_acc ? 1 : 0);
    const size_t padded = ((size_t)total_x + 1023) / 1024 * 1024;      // (a virtual thread adds zeros where the device's adds nothing: the same bits)
    scratch.resize(padded + 256);
    double* flat = scratch.data();
    double* acc = flat + padded;
    for (int slot = 0; slot <= a.n_out; slot++) out[slot] = 0.0;
    for (int slot = 0; slot < a.n_out; slot++) {
        bool fed = slot == 0;
        for (int k = 1; k < a.nacc && !fed; k++) fed = a.map[k - 1] == slot;
        if (fed) {
            for (int t = 0; t < 256; t++) acc[t] = 0.0;
            for (int k = 0; k < a.nacc; k++) {
                if (slot == 0 ? k != 0 : (k == 0 || a.map[k - 1] != slot)) continue;
                for (int c = 0; c < a.n_windows; c++)
                    for (int g = 0; g < G; g++) flat[(size_t)c * G + g] = a.sums[g * a.group_stride + (int64_t)c * a.nacc + k];
                if (a.lag_acc) flat[total] = a.lag_acc[k];
                for (size_t i = total_x; i < padded; i++) flat[i] = 0.0;
                for (size_t i0 = 0; i0 < padded; i0 += 1024) {       // (i0 < total_x: padded is total_x rounded up)
                    const double* f = flat + i0;
                    // (virtual thread t walks i0 + t while that is < total_x; past it the device's thread has left the loop)
                    const int live = (int)std::min<size_t>(256, (size_t)total_x - i0);
                    for (int t = 0; t < live; t++) acc[t] += (f[t] + f[t + 256]) + (f[t + 512] + f[t + 768]);
                }
            }
            for (int o = 128; o > 0; o >>= 1)
                for (int t = 0; t < o; t++) acc[t] += acc[t + o];
            out[slot] = acc[0];
        }
        for (int i = 0; i < 4; i++)
            if (a.add_slot[i] == slot) out[slot] += a.add[i];
    }
    uint64_t w = 0;
    for (int g = 0; g < G; g++) w = std::max(w, check_bits(a.chk[g * a.chk_stride]));
    if (a.lag_acc) w = std::max(w, check_bits(a.lag_chk));
    std::memcpy(&out[a.n_out], &w, 8);
}

// reduce_host where every record but group 0's and the by-value lag entry is zero (the head from its statistics: eval_iso): the
// same sums from those entries alone.  a.sums and a.chk are read for group 0 only.  Entry i of the device's order sits in the
// 1024-block i / 1024, on virtual thread i % 256, as term (i % 1024) / 256 of that thread's (v0 + v1) + (v2 + v3); the live entries
// are i = c G (window c) and i = n_windows G (the lag entry).  They are grouped by (block, thread) once, in ascending i -- a group is
// one addition of reduce_host --, then each fed slot adds its groups and runs the 256-wide tree whole.  Every addition reduce_host
// makes that is left out here adds +0.0, which changes no value (a sum that is -0.0 there may be +0.0 here or the reverse: equal
// by ==).  false, nothing written: more windows than REDUCE_HEAD_MAX_WINDOWS.
constexpr int REDUCE_HEAD_MAX_WINDOWS = 63;
inline bool reduce_host_head(const ReduceHostArgs& a, double* out) {
    if (a.n_windows > REDUCE_HEAD_MAX_WINDOWS) return false;
    const int n_live = a.n_windows + (a.lag_acc ? 1 : 0);
    struct Group { int64_t blk; int thr; int entry[4]; };          // entry[term]: the live entry that is this term, or -1
    Group grp[REDUCE_HEAD_MAX_WINDOWS + 1];
    int n_grp = 0;
    for (int e = 0; e < n_live; e++) {
        const int64_t i = (int64_t)e * a.n_groups;
        const int64_t blk = i / 1024;
        const int thr = (int)(i % 256), term = (int)(i % 1024) / 256;
        int g = 0;
        while (g < n_grp && (grp[g].blk != blk || grp[g].thr != thr)) g++;
        if (g == n_grp) { grp[n_grp++] = {blk, thr, {-1, -1, -1, -1}}; }
        grp[g].entry[term] = e;
    }
    double acc[256];
    for (int slot = 0; slot <= a.n_out; slot++) out[slot] = 0.0;
    for (int slot = 0; slot < a.n_out; slot++) {
        bool fed = slot == 0;
        for (int k = 1; k < a.nacc && !fed; k++) fed = a.map[k - 1] == slot;
        if (fed) {
            for (int t = 0; t < 256; t++) acc[t] = 0.0;
            for (int k = 0; k < a.nacc; k++) {
                if (slot == 0 ? k != 0 : (k == 0 || a.map[k - 1] != slot)) continue;
                for (int g = 0; g < n_grp; g++) {                  // (a thread's groups come block after block, as in reduce_host)
                    double v[4];
                    for (int u = 0; u < 4; u++) {
                        const int e = grp[g].entry[u];
                        v[u] = e < 0 ? 0.0 : e < a.n_windows ? a.sums[(int64_t)e * a.nacc + k] : a.lag_acc[k];
                    }
                    acc[grp[g].thr] += (v[0] + v[1]) + (v[2] + v[3]);
                }
            }
            for (int o = 128; o > 0; o >>= 1)
                for (int t = 0; t < o; t++) acc[t] += acc[t + o];
            out[slot] = acc[0];
        }
        for (int i = 0; i < 4; i++)
            if (a.add_slot[i] == slot) out[slot] += a.add[i];
    }
    uint64_t w = check_bits(a.chk[0]);
    if (a.lag_acc) w = std::max(w, check_bits(a.lag_chk));
    std::memcpy(&out[a.n_out], &w, 8);
    return true;
}

}  // namespace ssde_engine
#endif
