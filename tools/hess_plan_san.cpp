// hess_plan_san.cpp -- TEST INFRASTRUCTURE: the item plan and the retry rule of the Hessian pass (smoothsde_amd/csrc/ssde_windows.hpp:
// hess_first_warmup, hess_item_plan, hess_next_warmup) and knobs_from_env's SSDE_HESS_WINDOW under the sanitizers, as a program of
// its own
//     g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -o build/hess_plan_san tools/hess_plan_san.cpp && build/hess_plan_san
// on the inputs of tests/test_hess_plan_host.py: the track lengths 0 .. 3000, warm-ups 0, 16, 48, 80, 144 and 2^30 (whose quadruple
// no longer fits an int: the retry rule ends before it is formed), one and two pair blocks, wave budgets 1 .. 2^30.
#include <cstdio>
#include <cstdlib>

#include "../smoothsde_amd/csrc/ssde_knobs.hpp"
#include "../smoothsde_amd/csrc/ssde_windows.hpp"

using namespace ssde_engine;

struct Item { int32_t track, c, nc, b; };

int main() {
    const int WA = 16;
    long items_seen = 0, bad = 0;
    for (int W : {0, 16, 48, 80, 144}) {
        const std::vector<int32_t> L = {0, 1, 2, 15, 16, 17, 31, 32, 33, 2 * W - 1, 2 * W, 2 * W + 1, 640, 3000};
        for (int n_pb : {1, 2})
            for (int waves : {1, 64, 2048, 1 << 30}) {
                std::vector<Item> items;
                hess_item_plan(L, (int64_t)L.size(), n_pb, W, waves, WA, items);
                for (size_t k = 0; k < items.size(); k++) {
                    const Item& it = items[k];
                    items_seen++;
                    if (it.c + 1 < it.nc && (k + 1 >= items.size() || items[k + 1].track != it.track || items[k + 1].b != it.b || items[k + 1].c != it.c + 1)) bad++;
                    if (it.nc > 1 && L[(size_t)it.track] < 2 * W) bad++;
                }
            }
    }
    for (int W0 : {16, 48, 80, 144, 1 << 28})
        for (int glen : {0, 95, 96, 640, 3000, 1 << 30}) {
            int W = W0, n = 0;
            for (int attempt = 0; W != 0 && attempt < 10; attempt++, n++) W = hess_next_warmup(W, attempt, glen);
            if (W != 0 || n > 4) bad++;
        }
    if (hess_first_warmup(32, std::nullopt, WA) != 80 || hess_first_warmup(0, std::nullopt, WA) != 0 || hess_first_warmup(0, 16, WA) != 16) bad++;
    for (const char* v : {"0", "1", "16", "17", "2147483647", "-5", "junk"}) {
        setenv("SSDE_HESS_WINDOW", v, 1);
        const Knobs k = knobs_from_env(WA);
        if (!k.hess_window || *k.hess_window < WA || *k.hess_window % WA != 0 || *k.hess_window > (1 << 24)) bad++;
    }
    unsetenv("SSDE_HESS_WINDOW");
    if (knobs_from_env(WA).hess_window) bad++;
    printf("hess_plan_san: %ld items walked, %ld violations\n", items_seen, bad);
    return bad ? 1 : 0;
}
