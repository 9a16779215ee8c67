// A/B switches of the kernel launchers and the engine.  switches.def is the one table: a row per switch with its environment name,
// default, range, group and comment; the struct, the parser and the lookup by name below are generated from it.  TWO LIFETIMES, by
// the row's group.  CTX: cw_create parses the environment as it is then (read_switches()) into cw_ctx::sw, the context's own copy --
// setting the environment before Engine() selects it per context, which is how the differential tests build two engines in one
// process; cw_set_option and the hand-off fallback edit that copy.  LAUNCH: the launchers read the process table at every launch
// (cw_switches()); it starts as the environment of its first use (env_switches(), fixed for the process: a later change of the
// environment is ignored) and only cw_test_set_option edits it (set_test_option), between launches.  No launch path calls getenv or
// writes a switch.
#pragma once
#include <climits>

namespace cw_sw {

struct Switches {
#define CW_FLAG(field, env, group, rejected) bool field;
#define CW_NUM(field, env, dflt, range, group, rejected) int field;
#include "switches.def"
#undef CW_FLAG
#undef CW_NUM
};

enum Group { CTX, LAUNCH };
struct Row {
    const char* field;                 // name of the member of Switches, which is also the name the lookup takes
    const char* env;                   // environment variable, or null
    bool Switches::*flag;              // one of the two is set
    int Switches::*num;
    int dflt, lo, hi;
    bool reset;                        // out of [lo, hi]: the default (true) or the nearer bound
    Group group;
    bool rejected;
    int get(const Switches& s) const { return flag ? (int)(s.*flag) : s.*num; }
    void set(Switches& s, int v) const { if (flag) s.*flag = v != 0; else s.*num = v; }   // as given: the range is the parser's
};
extern const Row kRows[];
extern const int kNumRows;
const Row* find(const char* field);    // null: no such switch

Switches read_switches();              // the environment, parsed now
const Switches& env_switches();        // ... parsed on first use, then fixed for the process
const Switches& cw_switches();         // the process table the launchers read
// An option of cw_test_set_option that edits the process table (a value in the option's "environment" range restores
// env_switches()' value); false: no such option.
bool set_test_option(const char* option, int value);

}  // namespace cw_sw
