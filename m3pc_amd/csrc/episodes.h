// One episode store (include/m3pc_hip.h: m3pc_episodes_*), as episodes.hip keeps it and replay.hip reads it when it takes episodes
// over.  Device storage is allocated (and zeroed, in stream order) by the first call that enqueues work: m3pc_episodes_create itself
// makes no HIP call.
#pragma once
#include "stage.h"

struct m3pc_episodes {
    int device = 0, S = 0, A = 0, T = 0, n_envs = 0, M = 0;
    float *obs = nullptr, *act = nullptr, *rew = nullptr;  // (n_envs, M, S) (n_envs, M, A) (n_envs, M)
    int* len = nullptr;                                    // (n_envs,) path lengths
    bool ready = false;
    std::vector<int> mirror;     // path lengths as the calls made so far leave them
    std::vector<unsigned> seen;  // duplicate check of one call's ids: seen[e] == call
    unsigned call = 0;
    m3pc::StagePool pool;        // host arguments on their way to the device (stage.h)
};
