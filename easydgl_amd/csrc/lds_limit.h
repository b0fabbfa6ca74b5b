// The dynamic-LDS limit of a kernel, remembered per (kernel, device).  A kernel that asks for more dynamic LDS than the default
// limit must have the limit raised before the launch, and the runtime keeps that attribute PER DEVICE.  This header knows nothing
// of HIP: the caller passes the call that raises the limit (edgl_lds_limit in k_misc.hip owns the library's one table; the host
// test tests/host/lds_limit_main.cpp passes a counting fake).
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <utility>

// Launches at or below this many bytes of dynamic LDS need no attribute.
constexpr size_t EDGL_LDS_DEFAULT_LIMIT = 48 * 1024;

class LdsLimitMemo {
public:
    explicit LdsLimitMemo(size_t threshold = EDGL_LDS_DEFAULT_LIMIT) : threshold_(threshold) {}

    // Makes sure `kern` may be launched with `bytes` of dynamic LDS on device `dev`.  `set(kern, bytes)` raises the limit and returns
    // 0 on success; it runs only when `bytes` is above the threshold and above what was granted before.  A failure is returned
    // and not remembered, so the next call tries again.  dev < 0 (ordinal unknown): `set` runs every time, nothing is remembered.
    // Safe to call from any number of host threads: `set` runs under the lock, so what is recorded is what was granted last.
    template <typename Set>
    int ensure(const void* kern, int dev, size_t bytes, Set&& set) {
        if (bytes <= threshold_) return 0;
        if (dev < 0) return set(kern, bytes);
        std::lock_guard<std::mutex> lock(mu_);
        const auto key = std::make_pair(kern, dev);
        const auto it = granted_.find(key);
        if (it != granted_.end() && it->second >= bytes) return 0;
        const int err = set(kern, bytes);
        if (err == 0) granted_[key] = bytes;
        return err;
    }

private:
    const size_t threshold_;
    std::mutex mu_;
    std::map<std::pair<const void*, int>, size_t> granted_;
};
