// experimental_none.cpp — the product library's side of the experimental
// kernels: none is built, so every shape is refused.  The experimental
// library (make experimental) links pir_fused.hip and eval_trie.hip in this
// file's place.
#include "dpf_kernels.hpp"
#include "pir_kernels.hpp"

namespace dpfk {

bool pir_fused_built() { return false; }
bool pir_fused_ok(uint64_t, uint32_t, uint32_t, bool) { return false; }
hipError_t launch_pir_fused(const uint32_t*, uint32_t, uint32_t, uint32_t, uint64_t, const uint8_t*, uint64_t, uint32_t*,
                            uint32_t*, hipStream_t) {
    return hipErrorInvalidValue;
}

bool eval_trie_built() { return false; }
bool eval_trie_ok(uint32_t, uint32_t, uint64_t, uint32_t) { return false; }
hipError_t launch_eval_trie(const uint32_t*, uint32_t, uint32_t, const uint64_t*, uint64_t, uint64_t, const uint4*,
                            const uint8_t*, uint32_t, uint8_t*, hipStream_t) {
    return hipErrorInvalidValue;
}

}  // namespace dpfk
