// The switch table (switches.def) as data, its parser and the process table (see switches.h).
#include "switches.h"
#include <cstdlib>
#include <cstring>

namespace cw_sw {

#define SW_ANY INT_MIN, INT_MAX, false
#define SW_CLAMP(lo, hi) lo, hi, false
#define SW_RESET(lo, hi) lo, hi, true
#define CW_FLAG(field, env, group, rejected) {#field, env, &Switches::field, nullptr, 0, 0, 1, false, group, rejected != 0},
#define CW_NUM(field, env, dflt, range, group, rejected) {#field, env, nullptr, &Switches::field, dflt, range, group, rejected != 0},
const Row kRows[] = {
#include "switches.def"
};
const int kNumRows = (int)(sizeof(kRows) / sizeof(kRows[0]));

const Row* find(const char* field) {
    for (const Row& r : kRows) if (!strcmp(field, r.field)) return &r;
    return nullptr;
}

Switches read_switches() {
    Switches s{};
    for (const Row& r : kRows) {
        const char* v = r.env ? getenv(r.env) : nullptr;
        if (r.flag) { s.*r.flag = v != nullptr; continue; }
        // numeric switches are divisors / sizes in the launchers: keep them in the range the launch code is written for
        int x = v ? atoi(v) : r.dflt;
        if (x < r.lo) x = r.reset ? r.dflt : r.lo;
        if (x > r.hi) x = r.reset ? r.dflt : r.hi;
        s.*r.num = x;
    }
    return s;
}

const Switches& env_switches() {
    static const Switches s = read_switches();   // thread-safe one-time initialisation
    return s;
}

static Switches& process_table() {
    static Switches s = env_switches();
    return s;
}
const Switches& cw_switches() { return process_table(); }

bool set_test_option(const char* option, int value) {
    // values in [env_lo, env_hi] mean "as the environment says"; any other sets the field to the value (a flag: value != 0),
    // or for an option that names the opposite of its field to value == 0
    static const struct { const char* option; const char* field; bool inverted; int env_lo, env_hi; } opts[] = {
        {"gemm_pp", "no_gemm_pp", true, INT_MIN, -1},        {"gemm_8ph", "no_gemm_8ph", true, INT_MIN, -1},
        {"gemv_loop", "no_gemv_loop", true, INT_MIN, -1},    {"comb_rowgroups", "comb_no_rowgroups", true, INT_MIN, -1},
        {"gemm_w128", "gemm_w128", false, INT_MIN, -1},      {"beam_topk_1block", "beam_topk_1block", false, INT_MIN, -1},
        {"mt_variant", "mt_variant", false, -2, -2},         {"gemm256_min_tiles", "gemm256_min_tiles", false, 1, 0},
        {"cross_valu", "cross_valu", false, 0, 0},           {"cross_per_row", "cross_per_row", false, 0, 0},
        {"mel_valu", "mel_valu", false, INT_MIN, -1}};
    for (const auto& o : opts) {
        if (strcmp(option, o.option)) continue;
        const Row* r = find(o.field);
        const bool env = value >= o.env_lo && value <= o.env_hi;
        r->set(process_table(), env ? r->get(env_switches()) : o.inverted ? value == 0 : value);
        return true;
    }
    return false;
}

}  // namespace cw_sw
