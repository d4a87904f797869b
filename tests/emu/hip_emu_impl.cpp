// The one translation unit that carries the emulator's context-switch routine (test build only).
#define HIPEMU_IMPLEMENTATION
#include "hip_emu.h"

// test parameter of the CPU model: the compute units it reports (n < 1: back to the default of 8)
extern "C" __attribute__((visibility("default"))) void mi355vits_emu_set_cu_count(int n) {
    hipemu_cu_count.store(n >= 1 ? n : 8, std::memory_order_relaxed);
}
