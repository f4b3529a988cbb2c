// meshenv_grad_bind.h -- what every *_grad_bind of the loss-gradient handles refuses, written down once.
//
// Host-only and free of HIP: one GradBind row per bind says which tensor arrays the entry point takes and which of their
// tensors the kernels read 16 bytes at a time; grad_bind_refusal() turns a row and the caller's arguments into the text of
// *_last_error.  meshenv_hip.hip keeps the handles, the device guard and the allocation; tests/test_grad_bind_cpu.py
// compiles this header alone.
#pragma once

#include <cstdint>
#include <string>

namespace meshenv {

// One tensor array of a bind: w1 b1 w2 b2 ... in torch's layout.
struct GradBindNet {
    const char *noun;      // "null <noun>tensor": "actor ", "critic " or ""
    const char *weight;    // "<weight> tensor i is not 16-byte aligned"
    int count;             // tensors the array holds
    uint32_t aligned;      // bit i: tensor i is read 16 bytes at a time
};

struct GradBind {
    const char *fn;             // the entry point, in front of every refusal
    const char *takes, *shape;  // the refusal of a null array or a wrong count: what it takes, the supported shape
    const char *of, *at;        // "the gradient buffer<of> has N floats<at>, got M"
    int grad_align;             // bytes the gradient buffer is aligned to (a power of two)
    int n_nets;
    GradBindNet net[3];         // in argument order
};

// every weight behind the first layer's: even index >= 2
constexpr uint32_t grad_bind_inner_weights(int count) { return 0x55555554u & ((1u << count) - 1u); }

constexpr const char *kCriticGradKinds = "supported kinds: 0 (SAC: twin ReLU [128, 128, 128] critics) or 1 (TD3: twin ReLU [256, 256] critics); "
                                         "input cat(obs, action) = 21, float32";
constexpr const char *kPpoGradShapes = "supported: pi and vf towers of two hidden layers of the same width 64 or 128, activation 0 (ReLU) or 1 "
                                       "(Tanh), action_net [3], value_net [1], log_std [3], 18 observations, float32";
constexpr const char *kFnnShapes = "supported network: fc1 [64][18], fc2 [128][64], fc3 [64][128], fc4 [32][64], fc5 [16][32], action_head "
                                   "[2][16], type_head [3][16], each with a bias of its rows (general/EBRD.py Policy)";

// by kind: the hidden layers' [H][H] and the output layer's [1][H] weights
constexpr GradBind kCriticGradBind[2] = {
    {"meshenv_critic_grad_bind", "kind 0 takes 8 tensors per critic; ", kCriticGradKinds, " of kind 0", "", 1, 2,
     {{"critic ", "weight", 8, grad_bind_inner_weights(8)}, {"critic ", "weight", 8, grad_bind_inner_weights(8)}}},
    {"meshenv_critic_grad_bind", "kind 1 takes 6 tensors per critic; ", kCriticGradKinds, " of kind 1", "", 1, 2,
     {{"critic ", "weight", 6, grad_bind_inner_weights(6)}, {"critic ", "weight", 6, grad_bind_inner_weights(6)}}}};

// the [H][H] weights and the heads' [3][H] weights of the actor, then the twin critics
constexpr GradBind kActorGradBind = {
    "meshenv_actor_grad_bind", "takes 10 actor tensors and 8 tensors per critic ",
    "(SAC: actor ReLU [128, 128, 128] with mu / log_std heads, twin ReLU [128, 128, 128] critics, float32)", "", "", 1, 3,
    {{"actor ", "actor weight", 10, grad_bind_inner_weights(10)}, {"critic ", "critic weight", 8, grad_bind_inner_weights(8)},
     {"critic ", "critic weight", 8, grad_bind_inner_weights(8)}}};

// the [H][H] weights, the head's [3][H] and the critic's output [1][H] weights
constexpr GradBind kTd3ActorGradBind = {
    "meshenv_td3_actor_grad_bind", "takes 6 actor tensors and 6 tensors of the first critic ",
    "(TD3 / DDPG: actor ReLU [256, 256] with a Linear(256, 3) + Tanh head, critic ReLU [256, 256], float32)", "", "", 1, 2,
    {{"", "weight", 6, grad_bind_inner_weights(6)}, {"", "weight", 6, grad_bind_inner_weights(6)}}};

// w2 [300][400], the head's [3][300] and the critic's output [1][300] weights; the gradient buffer holds whole floats
constexpr GradBind kDdpgGradBind = {
    "meshenv_ddpg_grad_bind", "takes 6 actor tensors and 6 tensors of the critic ",
    "(DDPG: actor ReLU [400, 300] with a Linear(300, 3) + Tanh head, critic ReLU [400, 300], float32)", "", "", 4, 2,
    {{"", "weight", 6, grad_bind_inner_weights(6)}, {"", "weight", 6, grad_bind_inner_weights(6)}}};

// by width (64, 128): pi w1 b1 w2 b2 wh bh, vf likewise, log_std -- per tower the [H][H] and the head's [n_out][H] weights
constexpr uint32_t kPpoGradAligned = grad_bind_inner_weights(6) | grad_bind_inner_weights(6) << 6;
constexpr GradBind kPpoGradBind[2] = {
    {"meshenv_ppo_grad_bind", "takes 13 tensors: pi w1 b1 w2 b2 wh bh, vf w1 b1 w2 b2 wh bh, log_std", "", "", " at width 64", 1, 1,
     {{"", "weight", 13, kPpoGradAligned}}},
    {"meshenv_ppo_grad_bind", "takes 13 tensors: pi w1 b1 w2 b2 wh bh, vf w1 b1 w2 b2 wh bh, log_std", "", "", " at width 128", 1, 1,
     {{"", "weight", 13, kPpoGradAligned}}}};

// the weights behind fc1
constexpr GradBind kFnnGradBind = {"meshenv_fnn_grad_bind", "takes 14 tensors; ", kFnnShapes, "", "", 1, 1,
                                   {{"", "weight", 14, grad_bind_inner_weights(14)}}};

// What is wrong with a bind's arguments, as *_last_error reports it, or nothing.  tensors[k] and counts[k]: the caller's
// array and count of d.net[k] (an entry point without a count argument passes the row's); want: the floats of the gradient
// buffer.  Reads the arrays, never a tensor.
inline std::string grad_bind_refusal(const GradBind &d, const float *const *const *tensors, const int *counts, const float *grad_dev,
                                     int64_t n_grad, int64_t want)
{
    const std::string fn = std::string(d.fn) + ": ";
    for (int k = 0; k < d.n_nets; k++)
        if (!tensors[k] || counts[k] != d.net[k].count) return fn + d.takes + d.shape;
    if (!grad_dev || n_grad != want)
        return fn + "the gradient buffer" + d.of + " has " + std::to_string((long long)want) + " floats" + d.at + ", got " +
               std::to_string((long long)n_grad);
    for (int k = 0; k < d.n_nets; k++)
        for (int i = 0; i < d.net[k].count; i++) {
            if (!tensors[k][i]) return fn + "null " + d.net[k].noun + "tensor";
            if ((d.net[k].aligned >> i & 1u) && ((uintptr_t)tensors[k][i] & 15))
                return fn + d.net[k].weight + " tensor " + std::to_string(i) + " is not 16-byte aligned";
        }
    if ((uintptr_t)grad_dev & (uintptr_t)(d.grad_align - 1))
        return fn + "the gradient buffer is not " + std::to_string(d.grad_align) + "-byte aligned";
    return std::string();
}

// n (w, b) pairs out of a tensor array: w[l] = p[2 l], b[l] = p[2 l + 1]
inline void grad_bind_pairs(const float *const *p, int n, const float **w, const float **b)
{
    for (int l = 0; l < n; l++) {
        w[l] = p[2 * l];
        b[l] = p[2 * l + 1];
    }
}

}  // namespace meshenv
