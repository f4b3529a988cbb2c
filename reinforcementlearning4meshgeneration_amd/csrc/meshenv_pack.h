// meshenv_pack.h -- the packed-weight layout of the fused networks, once, for the host and the device.
//
// A network describes its buffer as a PackLayout: one PackSlot per source tensor (torch.nn.Linear layout: [out][in] row-major,
// [out] bias), in the order its *_bind takes them.  pack_host writes host tensors into a zero-filled host buffer by it (the
// *_load entry points, meshenv_fnn_pack); pack_table makes it the PackTable of live device tensors that k_target_pack copies in
// one launch (*_bind, *_refresh).  Neither writes what no source covers (the padding of K, of a head tile, of a bias block):
// the buffer is zeroed once.  The host half is plain C++.
#pragma once

#include <stddef.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MESHENV_PACK_HD __host__ __device__
#else
#define MESHENV_PACK_HD
#endif

namespace meshenv {

enum { kPackMatrix = 0, kPackVector = 1 };
constexpr int kTgtMaxCopies = 32;

struct PackCopy {
    const float *src;  // [out][in] row-major (matrix) or [out] (vector)
    float *dst;        // packed [tiles][groups][64][4] or a plain vector
    int out, in, groups, tiles;
    int n_off;         // first neuron (matrix) / first element (vector) of dst this source occupies
    int kind;
};

struct PackTable {
    PackCopy c[kTgtMaxCopies];
};

// Element i of a matrix copy's dst, in the per-lane MFMA B-operand order the forward kernels read: element j of lane l in group g
// of a 16-neuron tile holds W[n = 16 tile + (l & 15) - n_off][k = 4 (4 g + j) + (l >> 4)].  Elements outside the source (k >= in,
// neurons of another source or of the padding) are not written.
MESHENV_PACK_HD inline void pack_matrix_element(const PackCopy &c, int i)
{
    const int j = i & 3, lane = (i >> 2) & 63, tg = i >> 8;
    const int g = tg % c.groups, tile = tg / c.groups;
    const int k = 4 * (4 * g + j) + (lane >> 4), n = 16 * tile + (lane & 15) - c.n_off;
    if (k < c.in && n >= 0 && n < c.out) c.dst[i] = c.src[(size_t)n * c.in + k];
}

MESHENV_PACK_HD inline void pack_vector_element(const PackCopy &c, int i) { c.dst[c.n_off + i] = c.src[i]; }

struct PackSlot {      // a PackCopy without its pointers
    size_t off;        // of dst in the network's buffer
    int out, in, groups, tiles, n_off, kind;
};

struct PackLayout {
    PackSlot s[kTgtMaxCopies];
    int n = 0;
    size_t floats = 0;   // of the whole buffer

    void add(size_t off, int out, int in, int groups, int tiles, int n_off, int kind)
    {
        s[n++] = PackSlot{off, out, in, groups, tiles, n_off, kind};
    }
    // a new block at the end of the buffer with the source at its start; returns its offset
    size_t matrix(int out, int in, int groups, int tiles)
    {
        add(floats, out, in, groups, tiles, 0, kPackMatrix);
        floats += (size_t)tiles * groups * 256;
        return s[n - 1].off;
    }
    size_t vector(int out, int padded)
    {
        add(floats, out, 0, 0, 0, 0, kPackVector);
        floats += padded;
        return s[n - 1].off;
    }
    // One MLP tower: NL hidden layers of width H, the first over `in` inputs in `groups1` K groups, each with its bias; then a
    // 16-wide head tile and its bias, n_out columns, with `twin` a second head of as many behind them (SAC: mu, log_std).
    void tower(int H, int NL, int in, int groups1, int n_out, bool twin)
    {
        const int G = H / 16;
        matrix(H, in, groups1, G); vector(H, H);
        for (int l = 1; l < NL; l++) { matrix(H, H, G, G); vector(H, H); }
        const size_t wh = matrix(n_out, H, G, 1), bh = vector(n_out, 16);
        if (twin) { add(wh, n_out, H, G, 1, n_out, kPackMatrix); add(bh, n_out, 0, 0, 0, n_out, kPackVector); }
    }
    PackCopy copy(int i, const float *src, float *buf) const
    {
        return PackCopy{src, buf + s[i].off, s[i].out, s[i].in, s[i].groups, s[i].tiles, s[i].n_off, s[i].kind};
    }
};

// Host tensors src[0 .. L.n) into the zero-filled host buffer buf[L.floats]; a null source leaves its block zero.
inline void pack_host(const PackLayout &L, const float *const *src, float *buf)
{
    for (int s = 0; s < L.n; s++) {
        if (!src[s]) continue;
        const PackCopy c = L.copy(s, src[s], buf);
        if (c.kind == kPackVector)
            for (int i = 0; i < c.out; i++) pack_vector_element(c, i);
        else
            for (int i = 0; i < c.tiles * c.groups * 256; i++) pack_matrix_element(c, i);
    }
}

// The first n slots of L with the device tensors src_dev and the device buffer buf, as k_target_pack's argument.  Returns n.
inline int pack_table(const PackLayout &L, const float *const *src_dev, int n, float *buf, PackTable &T)
{
    for (int s = 0; s < n; s++) T.c[s] = L.copy(s, src_dev[s], buf);
    return n;
}

// blocks of 256 threads that cover the largest of T's first n copies in one pass: k_target_pack's grid is (this, n)
inline int pack_blocks(const PackTable &T, int n)
{
    int blocks = 1;
    for (int s = 0; s < n; s++)
        if (T.c[s].tiles * T.c[s].groups > blocks) blocks = T.c[s].tiles * T.c[s].groups;
    return blocks;
}

#ifdef __HIPCC__
// One launch copies every live tensor of the table into the handle's buffer; blockIdx.y selects the copy.
__global__ void __launch_bounds__(256)
k_target_pack(PackTable P)
{
    const PackCopy &c = P.c[blockIdx.y];
    const int stride = gridDim.x * 256, i0 = blockIdx.x * 256 + threadIdx.x;
    if (c.kind == kPackVector) {
        for (int i = i0; i < c.out; i += stride) pack_vector_element(c, i);
        return;
    }
    const int total = c.tiles * c.groups * 256;
    for (int i = i0; i < total; i += stride) pack_matrix_element(c, i);
}
#endif

}  // namespace meshenv
