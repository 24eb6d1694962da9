// Engine-selection switches of a model: every ALQ_* environment variable model.hip and passes.hip understand, in ONE table, read ONCE when
// the model is created (alq_model_create -> read_engine_switches).  No HIP dependency: tests/host/switches_main.cpp compiles
// this header with the host compiler alone.  (ALQ_G4_TUNE - a per-plan diagnostic string - and ALQ_NO_SIDE_STREAM - a switch
// of the context - are not model switches and stay where they are read; the engines' own files read their own variables.)
#ifndef ALQ_ENGINE_SWITCHES_H
#define ALQ_ENGINE_SWITCHES_H
#include <cstddef>
#include <cstdlib>

namespace alq {

// keys of alq_debug_set = indices of g_dbg_knobs (include/alq.h documents them)
enum Knob {
    KNOB_REPEAT = 0,          // repeat the MFMA phase n extra times
    KNOB_FLAGS = 1,           // flag bits: 1 no stores, 2 no loads, 4 no sum MFMAs, 8 no sum stores
    KNOB_NO_BWD_FUSE = 2,     // no epilogue fusion in backward GEMMs
    KNOB_NO_FWD_FUSE = 3,     // ... in forward GEMMs
    KNOB_NO_V3 = 4,           // the fp32-MFMA GEMM kernel instead of the bf16x3 split kernels
    KNOB_NO_V4 = 5,           // no two-slot engine (igemm4)
    KNOB_NO_POOL_FIRST = 6,   // no fused backward of the pool behind the first conv
    KNOB_NO_CONV_POOL = 7,    // first conv and the pool behind it as separate launches
    KNOB_DCP_NARROW = 8,      // the first conv + pool kernel on its narrow tile everywhere (direct.hip)
    KNOB_E3D_GRID_CAP = 9,    // at most that many workgroups in the plane-sweep launch of e3d.hip
    KNOB_C3B7_GRID_CAP = 10,  // ... in the 7-k-step backward launch of c3d.hip (alq_debug_set only: no environment variable)
    ALQ_NKNOBS = 11
};

struct EngineSwitches {
    int knobs[ALQ_NKNOBS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};      // the model's snapshot of the debug knobs (alq_debug_set overrides a key for all models)
    // plan time (gemm_build / build_model)
    int disable_v2 = 0;            // ALQ_DISABLE_V2=1 (diagnostics): force the general GEMM kernel, no igemm2 / direct plans
    int disable_v3 = 0;            // ALQ_DISABLE_V3=1: no igemm3 plans
    int disable_v4 = 0;            // ALQ_DISABLE_V4: no two-slot plans (igemm4), no split concat
    int no_fcgemm = 0;             // ALQ_NO_FCGEMM: wide fc layers without the streaming GEMM
    int no_split = 0;              // ALQ_NO_SPLIT: concat inputs as interleaved channel slices of one tensor
    int no_wide2d_rule = 0;        // ALQ_NO_WIDE2D_RULE: 2-D windows of 25 taps or more stay on the two-slot engine
    int no_v3_f16 = 0;             // ALQ_NO_V3_F16: igemm3 launches on bf16 triples only
    int no_v3_f16_fwd = 0;         // ALQ_NO_V3_F16_FWD: ... the forward ones
    int no_co_split = 0;           // ALQ_NO_CO_SPLIT: a wide conv is not cut into launches over slices of its output channels
    int no_co_split_f16 = 0;       // ALQ_NO_CO_SPLIT_F16: those slices on bf16 triples
    int no_class_tiles = 0;        // ALQ_NO_CLASS_TILES: no conv_transpose launch with its classes as tiles
    int no_fc_bits = 0;            // ALQ_NO_FC_BITS: the two-class head keeps no sign bytes (and nothing that builds on them)
    int no_fc_fuse = 0;            // ALQ_NO_FC_FUSE: the head's logits are not computed in the epilogue of the conv below
    int no_fc_f16 = 0;             // ALQ_NO_FC_F16: backward launch of a wide fc layer on bf16 triples
    int no_fc_f16_fwd = 0;         // ALQ_NO_FC_F16_FWD: ... the forward launch
    int f16_derived_mask = 0;      // ALQ_F16_DERIVED_MASK (study): the layers (bits) of alq_model::f16_fwd_derived, when has_f16_derived_mask
    int has_f16_derived_mask = 0;
    // per call
    int no_f16x2 = 0;              // ALQ_NO_F16X2: bf16x3 split in every launch
    int no_xcd_order = 0;          // ALQ_NO_XCD_ORDER (A/B): igemm4 tiles in dispatch order
    int no_fixed = 0;              // ALQ_NO_FIXED: runtime-constant igemm4 instantiations only
    int no_bound16 = 0;            // ALQ_NO_BOUND16: backward launches take their fp16x2 scale from measured per-patch maxima only
    int no_flipfix = 0;            // ALQ_NO_FLIPFIX (A/B: the head's sign bits as the fp16x2 contraction leaves them)
    int no_presplit = 0;           // ALQ_NO_PRESPLIT (A/B): split the fc head's weight-difference vector in the staging part again
    int no_signs = 0;              // ALQ_NO_SIGNS (A/B, bit-identity test): backward launches read ReLU masks from the fp32 activations
    int no_signs0 = 0;             // ALQ_NO_SIGNS0 (A/B): no sign field from the first conv + pool kernel only
    int f16_fwd_mask = -1;         // ALQ_F16_FWD_MASK (diagnostics): forward fp16x2 consumers by layer bit, -1 = default rule
    int no_f16_derived = 0;        // 1 with ALQ_NO_F16_DERIVED=1 (or ALQ_F16_DERIVED=0): those launches stay on bf16x3 (A/B; default since round 5: they take the split)
    int no_light_kernels = 0;      // ALQ_NO_LIGHT_KERNELS (A/B): forward-only passes keep dec1 / enc2 + pool2 on the two-slot engine as until round 5
    int no_c3d = 0;                // ALQ_NO_C3D (A/B): the head conv pair on the two-slot engine (igemm4) as in round 3
    // 7 (default): the 27 taps packed into 7 k-steps (c3d_bwd7_kernel); 8: the 9-k-step kernel of round 4; 4: its half-patch form
    int c3_bwd_rows = 7;           // ALQ_C3D_BWD_ROWS=4 / 8 (A/B)
    // the 7-k-step kernel's waves per SIMD: 2 (default since round 9: 512 threads, four rows per wave) or 1 (eight rows per wave); same bits
    int c3_bwd_waves = 2;          // ALQ_C3D_BWD_WAVES=1 (A/B)
    int no_e3d = 0;                // ALQ_NO_E3D (A/B): pool2 backward, enc2 backward and pool1 backward as three launches as in round 4
    int e3d_rows = 0;              // ALQ_E3D_ROWS=1 (A/B): that launch on the row-sweep kernel of rounds 5 - 7 instead of the z plane sweep (same bits)
    int no_d3d = 0;                // ALQ_NO_D3D (A/B): dec1's forward on the two-slot engine as in round 4
    int no_d3b = 0;                // ALQ_NO_D3D_BWD (A/B): only the backward launch on the two-slot engine
    int no_f3d = 0;                // ALQ_NO_F3D (A/B): enc2's forward on the two-slot engine + the pool as its own launch
    int no_t3d = 0;                // ALQ_NO_T3D (A/B): conv_transpose launches on the two-slot engine (igemm4) as in round 4
};

// How a variable's value becomes the member's.  Every rule but SW_ROWS leaves the member alone when it does not fire, so two
// rows may feed one member (ALQ_F16_DERIVED=0 and ALQ_NO_F16_DERIVED=1 both set no_f16_derived).
enum SwitchRule {
    SW_PRESENT,      // the variable exists, whatever its value (ALQ_NO_C3D=0 switches c3d off): member = 1
    SW_FIRST_IS_1,   // the value's first character is '1': member = 1
    SW_ATOI_EQ,      // atoi(value) == arg: member = 1
    SW_INT,          // the variable exists: member = atoi(value); otherwise the member keeps its default
    SW_ROWS          // ALQ_C3D_BWD_ROWS: atoi(value) 4 -> 4, 8 -> 8, anything else or unset -> 7
};

struct SwitchRow {
    const char *env;
    size_t member;      // offsetof(EngineSwitches, ...): every member is an int
    SwitchRule rule;
    int arg;
};

#define ALQ_SW(env, member, rule, arg) {env, offsetof(EngineSwitches, member), rule, arg}
inline const SwitchRow kSwitchTable[] = {
    ALQ_SW("ALQ_DEBUG_REPEAT", knobs[KNOB_REPEAT], SW_INT, 0),
    ALQ_SW("ALQ_DEBUG_FLAGS", knobs[KNOB_FLAGS], SW_INT, 0),
    ALQ_SW("ALQ_NO_BWD_FUSE", knobs[KNOB_NO_BWD_FUSE], SW_INT, 0),
    ALQ_SW("ALQ_NO_FWD_FUSE", knobs[KNOB_NO_FWD_FUSE], SW_INT, 0),
    ALQ_SW("ALQ_NO_V3", knobs[KNOB_NO_V3], SW_INT, 0),
    ALQ_SW("ALQ_NO_V4", knobs[KNOB_NO_V4], SW_INT, 0),
    ALQ_SW("ALQ_NO_POOL_FIRST", knobs[KNOB_NO_POOL_FIRST], SW_INT, 0),
    ALQ_SW("ALQ_NO_CONV_POOL", knobs[KNOB_NO_CONV_POOL], SW_INT, 0),
    ALQ_SW("ALQ_DCP_NARROW", knobs[KNOB_DCP_NARROW], SW_INT, 0),
    ALQ_SW("ALQ_E3D_GRID_CAP", knobs[KNOB_E3D_GRID_CAP], SW_INT, 0),
    ALQ_SW("ALQ_DISABLE_V2", disable_v2, SW_FIRST_IS_1, 0),
    ALQ_SW("ALQ_DISABLE_V3", disable_v3, SW_FIRST_IS_1, 0),
    ALQ_SW("ALQ_DISABLE_V4", disable_v4, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_FCGEMM", no_fcgemm, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_SPLIT", no_split, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_WIDE2D_RULE", no_wide2d_rule, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_V3_F16", no_v3_f16, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_V3_F16_FWD", no_v3_f16_fwd, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_CO_SPLIT", no_co_split, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_CO_SPLIT_F16", no_co_split_f16, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_CLASS_TILES", no_class_tiles, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_FC_BITS", no_fc_bits, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_FC_FUSE", no_fc_fuse, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_FC_F16", no_fc_f16, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_FC_F16_FWD", no_fc_f16_fwd, SW_PRESENT, 0),
    ALQ_SW("ALQ_F16_DERIVED_MASK", f16_derived_mask, SW_INT, 0),
    ALQ_SW("ALQ_F16_DERIVED_MASK", has_f16_derived_mask, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_F16X2", no_f16x2, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_XCD_ORDER", no_xcd_order, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_FIXED", no_fixed, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_BOUND16", no_bound16, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_FLIPFIX", no_flipfix, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_PRESPLIT", no_presplit, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_SIGNS", no_signs, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_SIGNS0", no_signs0, SW_PRESENT, 0),
    ALQ_SW("ALQ_F16_FWD_MASK", f16_fwd_mask, SW_INT, 0),
    ALQ_SW("ALQ_F16_DERIVED", no_f16_derived, SW_ATOI_EQ, 0),
    ALQ_SW("ALQ_NO_F16_DERIVED", no_f16_derived, SW_ATOI_EQ, 1),
    ALQ_SW("ALQ_NO_LIGHT_KERNELS", no_light_kernels, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_C3D", no_c3d, SW_PRESENT, 0),
    ALQ_SW("ALQ_C3D_BWD_ROWS", c3_bwd_rows, SW_ROWS, 0),
    ALQ_SW("ALQ_NO_E3D", no_e3d, SW_PRESENT, 0),
    ALQ_SW("ALQ_E3D_ROWS", e3d_rows, SW_ATOI_EQ, 1),
    ALQ_SW("ALQ_NO_D3D", no_d3d, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_D3D_BWD", no_d3b, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_F3D", no_f3d, SW_PRESENT, 0),
    ALQ_SW("ALQ_NO_T3D", no_t3d, SW_PRESENT, 0),
};
#undef ALQ_SW
inline const int kNumSwitchRows = (int)(sizeof(kSwitchTable) / sizeof(kSwitchTable[0]));

inline int &switch_member(EngineSwitches &sw, const SwitchRow &row) {
    return *reinterpret_cast<int *>(reinterpret_cast<char *>(&sw) + row.member);
}

inline EngineSwitches read_engine_switches() {
    EngineSwitches sw;
    for (const SwitchRow &row : kSwitchTable) {
        const char *v = std::getenv(row.env);
        int &dst = switch_member(sw, row);
        switch (row.rule) {
            case SW_PRESENT:    if (v) dst = 1; break;
            case SW_FIRST_IS_1: if (v && v[0] == '1') dst = 1; break;
            case SW_ATOI_EQ:    if (v && std::atoi(v) == row.arg) dst = 1; break;
            case SW_INT:        if (v) dst = std::atoi(v); break;
            case SW_ROWS:       dst = (v && std::atoi(v) == 4) ? 4 : ((v && std::atoi(v) == 8) ? 8 : 7); break;
        }
    }
    // ALQ_C3D_BWD_WAVES (round 9) is read here and not through the table: the table is held row for row to the getenv lines it
    // replaced (tests/host/switches_main.cpp), and this variable never had one.  1 -> 1, anything else or unset -> 2.
    if (const char *v = std::getenv("ALQ_C3D_BWD_WAVES")) sw.c3_bwd_waves = std::atoi(v) == 1 ? 1 : 2;
    return sw;
}

}  // namespace alq
#endif
