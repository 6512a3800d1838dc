// murmur3's 32-bit finaliser: the one mixing function of the library's counter-based generators (include/mdc.h states it under
// mdc_trainer_set_dropout).  train.hip draws its Dropout masks with it, iq_synth.hip everything a synthesised frame draws; both
// form draw j of a key as fmix32(key + j * 0xC2B2AE35).  A bijection of the 32-bit words; fmix32(0) == 0.
#pragma once

namespace mdc {

__host__ __device__ __forceinline__ unsigned fmix32(unsigned h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

}  // namespace mdc
