// Keyed sampling streams: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11 --
// the Random123 generator) and the maps from its 32-bit words to the numbers a sampling chain uses.  Every random
// number of a seeded chain is a pure function of (seed, item id, stream, step, position, block): no generator state,
// so a captured graph replays it and the draw of an item does not depend on the row it lands on ("Keyed
// sampling streams").  tests/test_keyed_rng_cpu.py restates all of this in numpy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// streams (counter word c2 = stream << 16 | step)
#define E3D_STREAM_STRUCT_XT 0      // structure x_T
#define E3D_STREAM_STRUCT_STEP 1    // structure reverse-step noise
#define E3D_STREAM_SEQ_XT 2         // sequence initial one-hot classes
#define E3D_STREAM_SEQ_U 3          // sequence posterior uniforms
// training and validation draws: the step field is the epoch, E3D_EPOCH_VALIDATION for validation
#define E3D_STREAM_TRAIN_STRUCT_T 4      // structure training timestep, class of T
#define E3D_STREAM_TRAIN_STRUCT_NOISE 5  // structure forward noise, laid out as stream 1
#define E3D_STREAM_TRAIN_SEQ_T 6         // sequence training timestep, class of T + 1
#define E3D_STREAM_TRAIN_SEQ_U 7         // sequence forward-noising uniform
#define E3D_EPOCH_VALIDATION 65535
// dropout decisions of a seeded training step: a row's key = words 0, 1 of (seed, item, stream, epoch, position, block 0).
// Streams 8 and 9 yield keys, not draws: E3D_STREAM_* above stays the list of the streams that draws are mapped from.
#define E3D_DROP_STREAM_LIGAND 8         // dropout on ligand rows (attention rows: the query's)
#define E3D_DROP_STREAM_POCKET 9         // dropout on pocket (receptor) rows
// partial redesign (replacement conditioning): the forward-noised copies of the held positions, step field = the chain's
// step index.  Named apart from E3D_STREAM_* like the dropout streams; streams 1 and 3 are untouched, so the free
// positions of a seeded chain make the draws they made before.
#define E3D_KNOWN_STREAM_STRUCT 10       // structure: forward noise of the held angles, laid out as stream 1
#define E3D_KNOWN_STREAM_SEQ 11          // sequence: forward-noising uniform of the held residues
// scoring supplied structures (stream 12): the forward noise of a supplied backbone at the level timestep t reads, step
// field = t, laid out as stream 1.  Stream 10 is not reused: it is drawn at the step whose LANDING level is t - 1, and has
// no draw for level T - 1.  (tests/test_score_cpu.py counts the *STREAM* macros above as the streams the sequence score
// left alone; this one is named apart from them.)
#define E3D_SCORE_STRUCT_NOISE 12

struct E3dU32x4 { uint32_t w[4]; };

__host__ __device__ __forceinline__ E3dU32x4 e3d_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                               uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    E3dU32x4 o;
    o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
    return o;
}

// The four words of (seed, item, stream, step, position, block).  Callers guarantee step <= 65535, 0 <= position < 2^24,
// block < 256 (checked on the host).
__device__ __forceinline__ E3dU32x4 e3d_keyed_words(uint64_t seed, uint64_t item, int stream, uint32_t step,
                                                    uint32_t position, uint32_t block) {
    return e3d_philox4x32_10((uint32_t)item, (uint32_t)(item >> 32), ((uint32_t)stream << 16) | step,
                             (position << 8) | block, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// uniform in [0, 1): the top 24 bits, exact in fp32
__device__ __forceinline__ float e3d_keyed_uniform(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }

// class in [0, C): ((w >> 8) * C) >> 24
__device__ __forceinline__ int e3d_keyed_class(uint32_t w, int C) { return (int)(((uint64_t)(w >> 8) * (uint32_t)C) >> 24); }

// Box-Muller on (w0, w1) and (w2, w3): z[0], z[1] from the first pair, z[2], z[3] from the second.
// u1 = ((w >> 8) + 1) 2^-24 in (0, 1], u2 = (w >> 8) 2^-24; r = sqrt(-2 ln u1); (r cos 2 pi u2, r sin 2 pi u2).
// Full-precision logf / sqrtf / sincospif: the result is a function of the words, not of fast-math choices.
__device__ __forceinline__ void e3d_keyed_normal4(const E3dU32x4 w, float (&z)[4]) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const float u1 = (float)((w.w[2 * p] >> 8) + 1u) * 0x1p-24f;
        const float u2 = e3d_keyed_uniform(w.w[2 * p + 1]);
        const float r = sqrtf(-2.0f * logf(u1));
        float s, c;
        sincospif(2.0f * u2, &s, &c);
        z[2 * p] = r * c;
        z[2 * p + 1] = r * s;
    }
}

// Row key table: int64 [rows, 2] = (item id, position); position < 0 marks a row of no item (a packed buffer's tail),
// which gets no draw.
#define E3D_KEY_SENTINEL (-1)
