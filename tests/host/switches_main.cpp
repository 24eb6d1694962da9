// Stand-alone check of csrc/engine_switches.h: every row of the switch table, under each of six settings of its variable,
// must give the member the value the getenv line it replaced gave it.  The expected values below are written out from those
// lines (alq_model_create, gemm_build and build_model before the table existed), not derived from the table's rules.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine_switches.h"

using namespace alq;

static const char *const kValues[6] = {nullptr, "", "0", "1", "4", "8"};      // nullptr = unset

struct Expect {
    const char *env;
    size_t member;
    int want[6];      // by kValues
};

#define M(m) offsetof(EngineSwitches, m)
#define PRESENT(env, m) {env, M(m), {0, 1, 1, 1, 1, 1}}      // getenv(env) != nullptr
#define KNOB(env, k) {env, M(knobs[k]), {0, 0, 0, 1, 4, 8}}  // if (v) knobs[k] = atoi(v)
static const Expect kExpect[] = {
    KNOB("ALQ_DEBUG_REPEAT", 0),
    KNOB("ALQ_DEBUG_FLAGS", 1),
    KNOB("ALQ_NO_BWD_FUSE", 2),
    KNOB("ALQ_NO_FWD_FUSE", 3),
    KNOB("ALQ_NO_V3", 4),
    KNOB("ALQ_NO_V4", 5),
    KNOB("ALQ_NO_POOL_FIRST", 6),
    KNOB("ALQ_NO_CONV_POOL", 7),
    KNOB("ALQ_DCP_NARROW", 8),
    KNOB("ALQ_E3D_GRID_CAP", 9),
    {"ALQ_DISABLE_V2", M(disable_v2), {0, 0, 0, 1, 0, 0}},      // e && e[0] == '1'
    {"ALQ_DISABLE_V3", M(disable_v3), {0, 0, 0, 1, 0, 0}},      // e && e[0] == '1'
    PRESENT("ALQ_DISABLE_V4", disable_v4),
    PRESENT("ALQ_NO_FCGEMM", no_fcgemm),
    PRESENT("ALQ_NO_SPLIT", no_split),
    PRESENT("ALQ_NO_WIDE2D_RULE", no_wide2d_rule),
    PRESENT("ALQ_NO_V3_F16", no_v3_f16),
    PRESENT("ALQ_NO_V3_F16_FWD", no_v3_f16_fwd),
    PRESENT("ALQ_NO_CO_SPLIT", no_co_split),
    PRESENT("ALQ_NO_CO_SPLIT_F16", no_co_split_f16),
    PRESENT("ALQ_NO_CLASS_TILES", no_class_tiles),
    PRESENT("ALQ_NO_FC_BITS", no_fc_bits),
    PRESENT("ALQ_NO_FC_FUSE", no_fc_fuse),
    PRESENT("ALQ_NO_FC_F16", no_fc_f16),
    PRESENT("ALQ_NO_FC_F16_FWD", no_fc_f16_fwd),
    {"ALQ_F16_DERIVED_MASK", M(f16_derived_mask), {0, 0, 0, 1, 4, 8}},      // if (e) f16_fwd_derived = atoi(e)
    PRESENT("ALQ_F16_DERIVED_MASK", has_f16_derived_mask),
    PRESENT("ALQ_NO_F16X2", no_f16x2),
    PRESENT("ALQ_NO_XCD_ORDER", no_xcd_order),
    PRESENT("ALQ_NO_FIXED", no_fixed),
    PRESENT("ALQ_NO_BOUND16", no_bound16),
    PRESENT("ALQ_NO_FLIPFIX", no_flipfix),
    PRESENT("ALQ_NO_PRESPLIT", no_presplit),
    PRESENT("ALQ_NO_SIGNS", no_signs),
    PRESENT("ALQ_NO_SIGNS0", no_signs0),
    {"ALQ_F16_FWD_MASK", M(f16_fwd_mask), {-1, 0, 0, 1, 4, 8}},         // if (f) f16_fwd_mask = atoi(f), default -1
    {"ALQ_F16_DERIVED", M(no_f16_derived), {0, 1, 1, 0, 0, 0}},         // e && atoi(e) == 0
    {"ALQ_NO_F16_DERIVED", M(no_f16_derived), {0, 0, 0, 1, 0, 0}},      // n && atoi(n) == 1
    PRESENT("ALQ_NO_LIGHT_KERNELS", no_light_kernels),
    PRESENT("ALQ_NO_C3D", no_c3d),
    {"ALQ_C3D_BWD_ROWS", M(c3_bwd_rows), {7, 7, 7, 7, 4, 8}},           // 4 -> 4, 8 -> 8, else 7
    PRESENT("ALQ_NO_E3D", no_e3d),
    {"ALQ_E3D_ROWS", M(e3d_rows), {0, 0, 0, 1, 0, 0}},                  // e && atoi(e) == 1
    PRESENT("ALQ_NO_D3D", no_d3d),
    PRESENT("ALQ_NO_D3D_BWD", no_d3b),
    PRESENT("ALQ_NO_F3D", no_f3d),
    PRESENT("ALQ_NO_T3D", no_t3d),
};
static const int kNumExpect = (int)(sizeof(kExpect) / sizeof(kExpect[0]));

static int g_failures = 0;

static void clear_all() {
    for (const SwitchRow &row : kSwitchTable) unsetenv(row.env);
}

static int member_at(const EngineSwitches &sw, size_t off) {
    int v;
    std::memcpy(&v, reinterpret_cast<const char *>(&sw) + off, sizeof(int));
    return v;
}

static void check(const char *what, int got, int want) {
    if (got == want) return;
    std::fprintf(stderr, "FAIL %s: got %d, want %d\n", what, got, want);
    ++g_failures;
}

// one or two variables set, everything else unset
static int with_env(const char *n1, const char *v1, const char *n2, const char *v2, size_t member) {
    clear_all();
    if (n1) setenv(n1, v1, 1);
    if (n2) setenv(n2, v2, 1);
    const EngineSwitches sw = read_engine_switches();
    clear_all();
    return member_at(sw, member);
}

int main() {
    // the table and the expectations cover each other row for row
    check("row count", kNumSwitchRows, kNumExpect);
    for (const SwitchRow &row : kSwitchTable) {
        int hits = 0;
        for (const Expect &e : kExpect) hits += std::strcmp(e.env, row.env) == 0 && e.member == row.member;
        char what[128];
        std::snprintf(what, sizeof(what), "expectations for table row %s", row.env);
        check(what, hits, 1);
    }
    for (const Expect &e : kExpect) {
        int hits = 0;
        for (const SwitchRow &row : kSwitchTable) hits += std::strcmp(e.env, row.env) == 0 && e.member == row.member;
        char what[128];
        std::snprintf(what, sizeof(what), "table row for expectation %s", e.env);
        check(what, hits, 1);
        for (int v = 0; v < 6; ++v) {
            std::snprintf(what, sizeof(what), "%s=%s", e.env, kValues[v] ? (kValues[v][0] ? kValues[v] : "\"\"") : "<unset>");
            check(what, with_env(kValues[v] ? e.env : nullptr, kValues[v], nullptr, nullptr, e.member), e.want[v]);
        }
    }
    // nothing set: the defaults
    {
        clear_all();
        const EngineSwitches sw = read_engine_switches(), def;
        check("defaults", std::memcmp(&sw, &def, sizeof(sw)), 0);
        check("default c3_bwd_rows", sw.c3_bwd_rows, 7);
        check("default f16_fwd_mask", sw.f16_fwd_mask, -1);
    }
    // the legacy oddities, one by one
    check("ALQ_NO_C3D=0 -> off", with_env("ALQ_NO_C3D", "0", nullptr, nullptr, M(no_c3d)), 1);
    check("ALQ_E3D_ROWS=2 -> 0", with_env("ALQ_E3D_ROWS", "2", nullptr, nullptr, M(e3d_rows)), 0);
    check("ALQ_C3D_BWD_ROWS=5 -> 7", with_env("ALQ_C3D_BWD_ROWS", "5", nullptr, nullptr, M(c3_bwd_rows)), 7);
    check("ALQ_F16_DERIVED=0 -> no_f16_derived", with_env("ALQ_F16_DERIVED", "0", nullptr, nullptr, M(no_f16_derived)), 1);
    check("ALQ_F16_DERIVED=1 ALQ_NO_F16_DERIVED=1", with_env("ALQ_F16_DERIVED", "1", "ALQ_NO_F16_DERIVED", "1", M(no_f16_derived)), 1);
    check("ALQ_F16_DERIVED=0 ALQ_NO_F16_DERIVED=0", with_env("ALQ_F16_DERIVED", "0", "ALQ_NO_F16_DERIVED", "0", M(no_f16_derived)), 1);
    check("ALQ_F16_DERIVED=1 ALQ_NO_F16_DERIVED=0", with_env("ALQ_F16_DERIVED", "1", "ALQ_NO_F16_DERIVED", "0", M(no_f16_derived)), 0);
    check("ALQ_DISABLE_V2=10 (first character)", with_env("ALQ_DISABLE_V2", "10", nullptr, nullptr, M(disable_v2)), 1);
    check("ALQ_DISABLE_V2=01", with_env("ALQ_DISABLE_V2", "01", nullptr, nullptr, M(disable_v2)), 0);
    check("ALQ_DISABLE_V3=yes", with_env("ALQ_DISABLE_V3", "yes", nullptr, nullptr, M(disable_v3)), 0);
    check("ALQ_NO_V4=x (atoi)", with_env("ALQ_NO_V4", "x", nullptr, nullptr, M(knobs[5])), 0);
    check("ALQ_F16_FWD_MASK=-1", with_env("ALQ_F16_FWD_MASK", "-1", nullptr, nullptr, M(f16_fwd_mask)), -1);
    if (g_failures) {
        std::fprintf(stderr, "%d failure(s)\n", g_failures);
        return 1;
    }
    std::printf("engine switches ok: %d rows x 6 settings\n", kNumExpect);
    return 0;
}
