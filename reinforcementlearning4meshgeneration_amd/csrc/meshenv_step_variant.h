// meshenv_step_variant.h -- which k_step / k_step_group instantiation a handle runs, written down once.
//
// Host-only and free of HIP: meshenv_hip.hip keeps two kernel-pointer arrays parallel to StepVariant and reads everything
// else -- the launch, the dynamic-LDS cap, meshenv_step_kernel / meshenv_rollout_kernel and the names they report -- from
// this header; tests/test_step_variant_cpu.py compiles it alone.  A new instantiation is one enum row, one table row, one
// pointer and, where it has a rule of its own, one line of select_step_variant.
#pragma once

namespace meshenv {

// What the choice depends on (MeshEnv fields; meshenv_hip.hip, step_facts).  Reachable inputs: group > 1 implies
// default_params, ragged implies group == 16.
struct StepFacts {
    bool multi;           // meshenv_rollout with n_steps > 1 (one launch, many steps)
    bool default_params;  // the geometry constants are the reference's: literal-constant instantiations
    bool front_moved;     // a front smoother ran since the last full reset: the tie-breaking instantiations
    int group;            // environments per workgroup of the single-step kernel: 1, 8 or 16
    bool ragged;          // CU-group LDS packed by each ring's own length
    int cap;              // ring stride in slots
    int stage_bits;       // bits 1 | 2 of k_step's auto_reset argument; bit 1 (record-first staging) selects kPre
};

// Rings of at most 64 slots: every ring pass is one 64-lane pass (the kSmall instantiations, k_step_group_actor's too).
constexpr bool step_small_ring(int cap) { return cap <= 64; }

enum StepVariant {
    // k_step_group<G, kDefaultParams, kRagged, kSmall>: one step, group > 1, not front_moved
    kGroupRagged16,
    kGroupSmall16,
    kGroupSmall8,
    kGroup16,
    kGroup8,
    // k_step<kMulti, kDefaultParams, kTie, kSmall, kPre>: one step
    kStepTie,
    kStepTieParams,
    kStepPreSmall,
    kStepPre,
    kStepSmall,
    kStepPlain,
    kStepParams,
    // the same kernel, n_steps > 1: group and stage_bits play no part
    kRolloutTie,
    kRolloutTieParams,
    kRolloutSmall,
    kRolloutPlain,
    kRolloutParams,
    kStepVariantCount
};
constexpr int kStepGroupVariants = kGroup8 + 1;                       // rows [0, 5): k_step_group
constexpr int kStepWaveVariants = kStepVariantCount - kStepGroupVariants;   // rows [5, 17): k_step

struct StepVariantRow {
    int code;          // what meshenv_step_kernel / meshenv_rollout_kernel return (include/meshenv.h)
    bool small;        // a kSmall instantiation: its dynamic LDS never passes 64 KB
    const char *name;  // the kernel as rocprofv3 prints it
};

constexpr StepVariantRow kStepVariants[kStepVariantCount] = {
    {4, false, "meshenv::k_step_group<16, true, true, false>"},
    {5, true, "meshenv::k_step_group<16, true, false, true>"},
    {5, true, "meshenv::k_step_group<8, true, false, true>"},
    {1, false, "meshenv::k_step_group<16, true, false, false>"},
    {1, false, "meshenv::k_step_group<8, true, false, false>"},
    {3, false, "meshenv::k_step<false, true, true, false, false>"},
    {10, false, "meshenv::k_step<false, false, true, false, false>"},
    {8, true, "meshenv::k_step<false, true, false, true, true>"},
    {7, false, "meshenv::k_step<false, true, false, false, true>"},
    {6, true, "meshenv::k_step<false, true, false, true, false>"},
    {0, false, "meshenv::k_step<false, true, false, false, false>"},
    {9, false, "meshenv::k_step<false, false, false, false, false>"},
    {3, false, "meshenv::k_step<true, true, true, false, false>"},
    {4, false, "meshenv::k_step<true, false, true, false, false>"},
    {1, true, "meshenv::k_step<true, true, false, true, false>"},
    {0, false, "meshenv::k_step<true, true, false, false, false>"},
    {2, false, "meshenv::k_step<true, false, false, false, false>"},
};

// After a front smoothing rings can hold vertices off the 1e-4 lattice, and with them clockwise angles exactly on a rounding
// boundary: until every env has been reset, steps run the one-wave-per-env kernel in its tie-breaking instantiation
// (csrc/meshenv_geom.h), whatever the group size.
constexpr StepVariant select_step_variant(const StepFacts &f)
{
    const bool small = step_small_ring(f.cap);
    if (!f.multi && f.group > 1 && !f.front_moved) {
        if (f.ragged) return kGroupRagged16;   // ragged: G == 16 only
        if (small) return f.group == 16 ? kGroupSmall16 : kGroupSmall8;
        return f.group == 16 ? kGroup16 : kGroup8;
    }
    if (f.multi) {
        if (f.front_moved) return f.default_params ? kRolloutTie : kRolloutTieParams;
        if (!f.default_params) return kRolloutParams;
        return small ? kRolloutSmall : kRolloutPlain;
    }
    if (f.front_moved) return f.default_params ? kStepTie : kStepTieParams;
    if (!f.default_params) return kStepParams;
    if (f.stage_bits & 2) return small ? kStepPreSmall : kStepPre;   // throughput regime only, decided in meshenv_create
    return small ? kStepSmall : kStepPlain;
}

}  // namespace meshenv
