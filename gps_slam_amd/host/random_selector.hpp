// gpsh::RandomSelector: the uniform branch of the reference's RandomSelector (include/dataset_reader.h:26-100) -- draw an index into
// the remaining list, take the element, swap with the back and pop, refill when empty -- with everything that the reference leaves
// to the platform written out, so that this class and its Python twin (gps_slam_amd/random_selector.py) give the same order:
//   * the generator is std::mt19937 seeded with the low 32 bits of `seed` (the reference seeds from std::random_device);
//   * the draw is NOT std::uniform_int_distribution (implementation-defined): one 32-bit output r at a time, rejected while
//     r >= 2^32 - 2^32 mod n, then r mod n -- unbiased on [0, n).
// gpsh::OptimScheduler: include/optim_scheduler.hpp of the reference with the gamma of raw_gs_model.cpp:673-674.
// Host code only: no device, no torch.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <random>
#include <stdexcept>
#include <vector>

namespace gpsh {

// unbiased draw on [0, n), n in [1, 2^32], from 32-bit outputs of `gen`
inline uint32_t drawBelow(std::mt19937& gen, uint64_t n) {
    const uint64_t zone = (uint64_t(1) << 32) - (uint64_t(1) << 32) % n;   // the largest multiple of n that fits
    for (;;) {
        const uint64_t r = (uint32_t)gen();
        if (r < zone) return (uint32_t)(r % n);
    }
}

template <class T>
class RandomSelector {
public:
    struct IndexedElement { const T* value; size_t originalIndex; };   // (the items are the caller's: they must outlive the selector)

    RandomSelector(const std::vector<T>& items, uint64_t seed) : gen_((uint32_t)(seed & 0xffffffffull)) {
        if (items.empty()) throw std::invalid_argument("RandomSelector: no items");
        for (size_t i = 0; i < items.size(); i++) original_.push_back({&items[i], i});
        current_ = original_;
    }
    IndexedElement getNext() {
        if (current_.empty()) current_ = original_;
        const size_t i = drawBelow(gen_, current_.size());
        const IndexedElement v = current_[i];
        current_[i] = current_.back();
        current_.pop_back();
        return v;
    }

private:
    std::vector<IndexedElement> original_, current_;
    std::mt19937 gen_;
};

// meansOptScheduler: lr *= gamma per step, gamma = std::pow(0.01, 1.0f / max_iterations) -- a FLOAT quotient and a double pow, as
// the reference writes it; max_iterations <= 0: no scheduler, step() leaves the rate alone
struct OptimScheduler {
    bool active = false;
    double gamma = 1.0;
    OptimScheduler() = default;
    explicit OptimScheduler(int max_iterations) : active(max_iterations > 0) {
        if (active) gamma = std::pow(0.01, 1.0f / max_iterations);
    }
    void step(double& lr) const { if (active) lr = lr * gamma; }
};

}  // namespace gpsh
