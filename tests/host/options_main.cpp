// options_main.cpp — csrc/th_options.h on its own (tests/test_host_options.py builds and drives this).  `options_main names` prints the table's names, one per line.
// `options_main 0|1` (the argument: is this the EXPERIMENTS build?) reads lines `name prime value` and, on a fresh Options for each, applies `prime` (a value the option
// takes), then `value`, and prints `rc<TAB>field before<TAB>field after<TAB>message`; an unknown name prints the fields as `-`.
#include "../../trace.jl_amd/csrc/th_options.h"

#include <cinttypes>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (!std::strcmp(argv[1], "names")) {
        for (const OptionRow& r : kOptionRows) std::puts(r.name);
        return 0;
    }
    const bool experiments = std::atoi(argv[1]) != 0;
    char name[128];
    long long prime, value;
    while (std::scanf("%127s %lld %lld", name, &prime, &value) == 3) {
        Options o;
        char msg[512] = "";
        const OptionRow* r = find_option(name);
        if (r && apply_option(o, true, name, prime, msg, sizeof msg) != 0) {
            std::printf("prime refused: %s\n", msg);
            return 1;
        }
        msg[0] = 0;
        const int64_t before = r ? r->field.load(o) : 0;
        const int rc = apply_option(o, experiments, name, value, msg, sizeof msg);
        if (r)
            std::printf("%d\t%" PRId64 "\t%" PRId64 "\t%s\n", rc, before, r->field.load(o), msg);
        else
            std::printf("%d\t-\t-\t%s\n", rc, msg);
        if (option_in_build(experiments, name, value) != (experiments || rc != TRHIP_ERR_UNSUPPORTED)) {
            std::printf("option_in_build disagrees with apply_option for %s = %lld\n", name, value);
            return 1;
        }
    }
    return 0;
}
