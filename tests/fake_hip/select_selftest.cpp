// TEST-ONLY driver of qdsp_amd/csrc/select.cpp (with knobs.cpp), built by g++ with -fsanitize=address,undefined: no GPU, no HIP.
//
//     select_selftest MAP            recompute every line of the dispatch map (tests/golden/dispatch_map.txt, written by
//                                    scripts/dispatch_map.py from the library's own calls on a GPU) with plan_of() and select();
//                                    fail on the first line that differs.  Also checks what the map must cover: every kernel
//                                    family, and every setting 1-8 of the decimators' exception table.
//     select_selftest MAP --write    print the map as the selector computes it (same rows), for a change that retunes on purpose
//
// A line reads `settings class L M taps | count=family ... end=count` (scripts/dispatch_map.py); the ladder of call sizes and the
// variables of the `parity` and `setting7` rows below are that script's.
#include "../../qdsp_amd/csrc/knobs.h"
#include "../../qdsp_amd/csrc/select.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

using namespace qh;

namespace {

const char* const kParity[5][2] = {{"QDSP_HIP_MF_MIN_COUNT", "0"}, {"QDSP_HIP_RM_MIN_COUNT", "0"}, {"QDSP_HIP_FFT1K_MAX_COUNT", "0"},
                                   {"QDSP_HIP_NO_LM_SMALL_CALL_RULE", "1"}, {"QDSP_HIP_DECIM_SETTING", "0"}};

std::vector<int64_t> ladder() {      // 2^{6, 10, 12, 14, 16, 18, 19 .. 27} and 1 000 000, ascending
    std::vector<int64_t> v;
    for (int k : {6, 10, 12, 14, 16, 18, 19}) v.push_back(int64_t(1) << k);
    v.push_back(1000000);
    for (int k = 20; k <= 27; k++) v.push_back(int64_t(1) << k);
    return v;
}

bool describe(const std::string& cls, int L, int M, int taps, HandleDesc* d) {
    std::string base = cls;
    int mode = 0;
    const size_t colon = cls.find(':');
    if (colon != std::string::npos) {
        base = cls.substr(0, colon);
        const std::string m = cls.substr(colon + 1);
        mode = m == "direct" ? 1 : m == "fft" ? 2 : -1;
        if (mode < 0) return false;
    }
    d->L = L;
    d->M = M;
    d->ntaps = taps;
    d->P = L > 0 ? (taps + L - 1) / L : 0;
    d->fir_mode = mode;
    d->rotate = false;
    d->has_filter = true;
    d->ch = 2;
    if (base == "fir_c") d->kind = KIND_FIR;
    else if (base == "fir_r") { d->kind = KIND_FIR; d->ch = 1; }
    else if (base == "dec_c" || base == "rat_c") d->kind = KIND_DECIM;
    else if (base == "dec_r" || base == "rat_r") { d->kind = KIND_DECIM; d->ch = 1; }
    else if (base == "vfo") { d->kind = KIND_VFO; d->rotate = true; }
    else if (base == "xlate") { d->kind = KIND_XLATE; d->rotate = true; d->has_filter = false; }
    else return false;
    return true;
}

// the name last_kernel() reports for the family, folded as tests/conftest.py kname() folds it
const char* kernel_name(Family f, const HandleDesc& d) {
    const bool real = d.ch == 1;
    switch (f) {
    case F_XLATE: return "xlate_kernel";
    case F_FIR_LAT: return "fir_lat_kernel";
    case F_MFMA_DECIM: return real ? "decim_mfma_real_kernel" : "decim_mfma_kernel";
    case F_PFB: return d.M == 4 ? (real ? "pfb_dec4_real_kernel" : "pfb_dec4_kernel") : (real ? "pfb_dec8_real_kernel" : "pfb_dec8_kernel");
    case F_FFT1K: return "fir_fft1k_kernel";
    case F_FFT4K: return "fir_fft_kernel";
    case F_WIN: return "decim_win_kernel";
    case F_CORE: return "fir_core_kernel";
    case F_MFMA_RATIONAL: return real ? "resamp_mfma_real_kernel" : "resamp_mfma_kernel";
    case F_LM: return "resamp_lm_kernel";
    case F_ANY: return "resamp_any_kernel";
    }
    return "?";
}

void apply_settings(const std::string& name) {
    for (const auto& kv : kParity) {
        if (name == "parity") setenv(kv[0], kv[1], 1);
        else unsetenv(kv[0]);
    }
    if (name == "setting7") setenv("QDSP_HIP_DECIM_SETTING", "7", 1);      // (the committed table holds no 7: scripts/dispatch_map.py)
    qk::knobs_reload();
}

}  // namespace

// knobs_reload() keeps superseded snapshots alive on purpose (knobs.h: a reader that holds one stays valid): not a leak to report
extern "C" const char* __lsan_default_suppressions() { return "leak:knobs_reload\n"; }

int main(int argc, char** argv) {
    if (argc < 2) { printf("usage: select_selftest MAP [--write]\n"); return 2; }
    const bool write = argc > 2 && !strcmp(argv[2], "--write");
    {   // the switches are this program's to set: none comes in from outside
        std::vector<std::string> names;
        for (char** e = environ; e && *e; e++)
            if (!strncmp(*e, "QDSP_HIP_", 9)) names.push_back(std::string(*e, strcspn(*e, "=")));
        for (const std::string& n : names) unsetenv(n.c_str());
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) { printf("FAIL: cannot read %s\n", argv[1]); return 1; }
    const std::vector<int64_t> rungs = ladder();
    std::set<std::string> families;
    std::set<std::pair<int, int>> exceptions;      // (veto, mode) pairs met outside `parity` (which switches the table off): one per table setting
    std::string settings_now;
    char buf[4096];
    int lineno = 0, rows = 0;
    while (fgets(buf, sizeof(buf), f)) {
        lineno++;
        std::string line(buf);
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (line.empty() || line[0] == '#') {
            if (write) printf("%s\n", lineno == 1 ? "# dispatch map as qdsp_amd/csrc/select.cpp computes it: tests/fake_hip/select_selftest.cpp --write" : line.c_str());
            continue;
        }
        char settings[32], cls[32];
        int L, M, taps;
        long long end = 0;
        const size_t bar = line.find(" | "), endpos = line.rfind(" end=");
        if (bar == std::string::npos || endpos == std::string::npos || sscanf(line.c_str(), "%31s %31s %d %d %d", settings, cls, &L, &M, &taps) != 5 ||
            sscanf(line.c_str() + endpos, " end=%lld", &end) != 1) {
            printf("FAIL line %d: not a map line: %s\n", lineno, line.c_str());
            return 1;
        }
        HandleDesc d;
        if (!describe(cls, L, M, taps, &d) || (strcmp(settings, "default") && strcmp(settings, "parity") && strcmp(settings, "setting7"))) {
            printf("FAIL line %d: unknown class or settings: %s\n", lineno, line.c_str());
            return 1;
        }
        if (settings_now != settings) {
            settings_now = settings;
            apply_settings(settings_now);
        }
        const Plan plan = plan_of(d);
        std::string got = line.substr(0, bar) + " |";
        const char* prev = nullptr;
        for (int64_t count : rungs) {
            if (count > end) break;
            const char* name = kernel_name(select(d, plan, count), d);
            families.insert(name);
            if (settings_now != "parity") {
                const Exceptions x = call_exceptions(d, count);
                exceptions.insert({x.veto, x.mode});
            }
            if (!prev || strcmp(prev, name)) got += " " + std::to_string((long long)count) + "=" + name;
            prev = name;
        }
        got += " end=" + std::to_string(end);
        rows++;
        if (write) {
            printf("%s\n", got.c_str());
        } else if (got != line) {
            printf("FAIL line %d: the selector and the map differ\n  map:      %s\n  selector: %s\n", lineno, line.c_str(), got.c_str());
            return 1;
        }
    }
    fclose(f);
    if (write) return 0;
    if (rows == 0) { printf("FAIL: no rows in %s\n", argv[1]); return 1; }
    static const char* const kAll[] = {"xlate_kernel", "fir_lat_kernel", "fir_core_kernel", "fir_fft1k_kernel", "fir_fft_kernel", "decim_win_kernel",
                                       "decim_mfma_kernel", "decim_mfma_real_kernel", "pfb_dec8_kernel", "pfb_dec4_kernel", "pfb_dec8_real_kernel",
                                       "pfb_dec4_real_kernel", "resamp_mfma_kernel", "resamp_mfma_real_kernel", "resamp_lm_kernel", "resamp_any_kernel"};
    for (const char* name : kAll)
        if (!families.count(name)) { printf("FAIL: no row of the map reaches %s\n", name); return 1; }
    // settings 1-8 of decim_table.inc as (veto, mode) (kDecimSettingVeto / kDecimSettingMode, select.cpp)
    static const int kSettings[8][2] = {{VETO_WIN, 0}, {VETO_FFT1K, 0}, {VETO_WIN | VETO_FFT1K, 0}, {0, 1}, {0, 2}, {VETO_PFB, 0}, {VETO_PFB, 2}, {VETO_MF, 0}};
    for (int k = 0; k < 8; k++)
        if (!exceptions.count({kSettings[k][0], kSettings[k][1]})) { printf("FAIL: no row of the map meets setting %d of the decimators' table\n", k + 1); return 1; }
    printf("select ok: %d rows, %zu families\n", rows, families.size());
    return 0;
}
