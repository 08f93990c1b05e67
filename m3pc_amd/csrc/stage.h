// Host data on its way to the device, for the objects whose calls never wait for it (the episode store, the replay buffer): ids, host
// observations / actions / rewards / tables / indices are copied into a pinned, device-visible block the kernel reads directly.  A
// block is taken again once the event behind its last reader has completed; while none is free another one is allocated -- the host
// never waits for the device.
#pragma once
#include "m3pc_internal.h"

namespace m3pc {

struct StagePool {
    struct Stage {
        void *host = nullptr, *dev = nullptr;
        size_t bytes = 0;
        hipEvent_t ev = nullptr;
    };
    std::vector<Stage> stages;
    std::vector<int> held;  // blocks the call being enqueued reads

    // a block of at least `bytes` that no enqueued work reads: its host address in *host, its device view in *dev; valid until
    // the work enqueued by this call has run
    int take(size_t bytes, void** host, const void** dev, const char* who) {
        int pick = -1;
        for (size_t s = 0; s < stages.size() && pick < 0; ++s) {
            const auto& g = stages[s];
            if (g.bytes >= bytes && std::find(held.begin(), held.end(), (int)s) == held.end() && hipEventQuery(g.ev) == hipSuccess) pick = (int)s;
        }
        (void)hipGetLastError();  // (hipErrorNotReady of a busy block is not an error of the call)
        if (pick < 0) {
            Stage g;
            g.bytes = 4096;
            while (g.bytes < bytes) g.bytes *= 2;
            HIPCHK(hipHostMalloc(&g.host, g.bytes, hipHostMallocMapped));
            if (hipHostGetDevicePointer(&g.dev, g.host, 0) != hipSuccess || hipEventCreateWithFlags(&g.ev, hipEventDisableTiming) != hipSuccess) {
                (void)hipHostFree(g.host);
                return fail(M3PC_EHIP, "%s: no device view of a %zu-byte staging block", who, g.bytes);
            }
            stages.push_back(g);
            pick = (int)stages.size() - 1;
        }
        held.push_back(pick);
        *host = stages[pick].host;
        *dev = stages[pick].dev;
        return 0;
    }

    // `bytes` of host memory -> a device-visible address that stays valid until the work enqueued by this call has run
    int stage(const void* src, size_t bytes, const void** dev, const char* who) {
        void* host = nullptr;
        CHK(take(bytes, &host, dev, who));
        memcpy(host, src, bytes);
        return 0;
    }

    // behind the launch that reads them: the call's blocks become free again when `st` has passed this point
    int release(hipStream_t st) {
        for (int s : held) HIPCHK(hipEventRecord(stages[s].ev, st));
        held.clear();
        return 0;
    }

    // (the owner has drained the device)
    void destroy() {
        for (auto& g : stages) {
            (void)hipEventDestroy(g.ev);
            (void)hipHostFree(g.host);
        }
        stages.clear();
        held.clear();
    }
};

}  // namespace m3pc
