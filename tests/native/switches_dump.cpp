// Driver of tests/test_switches_host.py: prints every field of read_switches() by walking the table, then applies the
// option=value pairs of argv to the process table (cw_sw::set_test_option) and prints the table after each one.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../crisperwhisper_amd/csrc/switches.h"

static void dump(const cw_sw::Switches& s) {
    for (int i = 0; i < cw_sw::kNumRows; ++i) printf("%s=%d\n", cw_sw::kRows[i].field, cw_sw::kRows[i].get(s));
}

int main(int argc, char** argv) {
    printf("# environment\n");
    dump(cw_sw::read_switches());
    for (int i = 1; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string name(argv[i], (size_t)(eq - argv[i]));
        const bool ok = cw_sw::set_test_option(name.c_str(), atoi(eq + 1));
        printf("# %s %s\n", argv[i], ok ? "ok" : "rejected");
        dump(cw_sw::cw_switches());
    }
    return 0;
}
