// The noise of the train-time augmentation chain (train_augment.hip): a stateless hash, so that a batch's noise depends
// on (seed, counter, image row, element) alone.  train_augment.noise_normal (Python, numpy) is the specification.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dfd {

// MurmurHash3's 32-bit finaliser
__host__ __device__ inline uint32_t aug_fmix32(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    return x ^ (x >> 16);
}

// key of one image of one call: the chain of head_train.hip's dropout key with the image row in the layer's place
__host__ __device__ inline uint32_t aug_noise_key(unsigned long long seed, unsigned long long counter, int row) {
    uint32_t k = aug_fmix32((uint32_t)seed + 0x9E3779B9u);
    k = aug_fmix32(k ^ (uint32_t)(seed >> 32));
    k = aug_fmix32(k ^ (uint32_t)counter);
    k = aug_fmix32(k ^ (uint32_t)(counter >> 32));
    return aug_fmix32(k ^ (uint32_t)(row + 1));
}

// the two uniform words of element e
__host__ __device__ inline uint32_t aug_noise_word(uint32_t key, uint32_t idx) { return aug_fmix32(aug_fmix32(idx ^ key) + key); }

}  // namespace dfd
