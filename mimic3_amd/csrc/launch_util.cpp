// launch_util.cpp — what the launchers share: the compute-unit count behind every persistent grid, the large-LDS opt-in, and the
// host half of items.h (the items of a ragged batch that have work, and the grid and item order of a persistent launch over them).
#include <atomic>
#include <mutex>
#include <set>
#include <vector>

#include "items.h"
#include "kernels.h"

namespace m355 {

int valid_items(const int* len_host, const int* len_dev, int B, int T, int block, int extra) {
    if (B <= 0 || T <= 0 || block <= 0) return 0;
    const int full = (T + block - 1) / block;
    if (!len_dev) return B * full;
    std::vector<int> tmp;
    if (!len_host) {
        tmp.resize((size_t)B);
        HIP_CHECK(hipMemcpy(tmp.data(), len_dev, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost));
        len_host = tmp.data();
    }
    long n = 0;
    for (int b = 0; b < B; ++b) {
        const int ln = len_host[b] <= 0 ? 0 : (len_host[b] + extra > T ? T : len_host[b] + extra);
        if (ln > 0) n += (ln + block - 1) / block;
    }
    return (int)n;
}

ItemLaunch item_launch(const int* len_host, const int* len_dev, int B, int T, int N, int extra, int cus, int order) {
    ItemLaunch l;
    l.nvalid = valid_items(len_host, len_dev, B, T, N, extra);
    l.grid = l.nvalid < cus ? l.nvalid : cus;  // persistent: one workgroup per CU
    l.item_order = item_order_rule(order, l.nvalid, l.grid);
    return l;
}

// the > 64 KiB dynamic-LDS opt-in is a per-device function attribute: once per (kernel, device)
void set_max_dynamic_lds(const void* fn, int bytes) {
#ifndef MI355_EMU
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({fn, dev})) return;
    HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert({fn, dev});
#else
    (void)fn; (void)bytes;
#endif
}

// the one lookup of the compute-unit count behind every persistent grid and every form chosen by grid size
int current_device_cu_count() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
#ifdef MI355_EMU
    // the CPU model's count is a test parameter (mi355vits_emu_set_cu_count): read at every launch, never cached
    hipDeviceProp_t p;
    return (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
#else
    static std::atomic<int> cached[64];  // looked up once per device
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n <= 0) {
        hipDeviceProp_t p;
        n = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
#endif
}

}  // namespace m355
