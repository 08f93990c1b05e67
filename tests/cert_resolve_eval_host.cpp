// cert_resolve_eval of m3pc_amd/csrc/cert_resolve.h (the protocol loop with the eval_action certificate behind it) driven without a
// device: scripted certificates and scripted bounds in, the trace of ops calls and both records out
// (tests/test_cert_resolve_eval_cpu.py holds the expected traces).
//
// stdin, per scenario:   name N kmax rmax n_done r_done delta grow eval_tol n_reads n_bounds
//                        n_reads lines     deviation need need_race
//                        n_bounds numbers  b0: the bound the next bound kernel finds at n = n_done
// The fake bound kernel: bound(n') = b0 2^-(n' - n) for n <= n' <= n_listed; need_eval = the smallest such n' with bound(n') <=
// eval_tol, or N when there is none -- what the device kernel reports, on a bound that halves with every listed entry.
// The fake ops also play the pipelined step's launch in advance: a block for (r_done, n_done, min(kmax, N), delta) as they come
// in, valid while no merge has been issued; eval_read prints whether it took it.
// Read i (from 0) carries shift = (i + 1) / 8 and margin = (i + 1) / 16, so the record shows which read came last.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <iostream>
#include <string>
#include <vector>

#include "cert_resolve.h"
#include "m3pc_hip.h"

using m3pc::CertState;
using m3pc::EvalState;

struct Read {
    float deviation;
    int need, need_race;
};

struct FakeOps {
    CertState& s;
    float eval_tol;
    std::vector<Read> reads;
    std::vector<float> bounds;
    size_t next = 0, next_bound = 0;
    int merges = 0;  // issued behind the first pass
    bool spec = true;
    int spec_n_listed = 0;
    double spec_delta = 0.0;
    int read(bool four_only, float* out8) {
        printf("read %d\n", (int)four_only);
        if (next == reads.size()) return 99;  // the script is exhausted: the loop asked for more than the scenario foresaw
        const Read& r = reads[next++];
        const float v[8] = {(float)next / 8.f, r.deviation, (float)r.need, (float)next / 16.f, 0.f, (float)r.need_race, 0.f, 0.f};
        std::copy(v, v + 8, out8);
        return 0;
    }
    int eval_read(int n_listed, float* out8) {
        const bool take = spec && merges == 0 && n_listed == spec_n_listed && s.delta == spec_delta;
        spec = false;
        printf("eval_read %d %d %d %.17g %d\n", n_listed, s.r_done, s.n_done, s.delta, (int)take);
        if (next_bound == bounds.size()) return 98;
        const float b0 = bounds[next_bound++];
        int need = s.N;
        float b = b0;
        for (int n = s.n_done; n <= n_listed; ++n, b *= 0.5f)
            if (b <= eval_tol) {
                need = n;
                break;
            }
        const float v[8] = {b0, (float)need, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        std::copy(v, v + 8, out8);
        return 0;
    }
    int extend(int lo, int hi) { return printf("extend %d %d\n", lo, hi), 0; }
    int extend_race(int lo, int hi) { return printf("extend_race %d %d\n", lo, hi), 0; }
    int window_set(int need, bool everything) {
        printf("window_set %d %d %.17g\n", need, (int)everything, s.delta);
        s.n_done = everything ? s.N : std::min(need, s.N);
        ++merges;
        return 0;
    }
    int merge_select() {
        ++merges;
        return printf("merge_select %d %d %.17g\n", s.n_done, s.r_done, s.delta), 0;
    }
};

int main() {
    std::string name;
    while (std::cin >> name) {
        int N, kmax, rmax, n_done, r_done, grow, n_reads, n_bounds;
        double delta;
        std::string tol;
        if (!(std::cin >> N >> kmax >> rmax >> n_done >> r_done >> delta >> grow >> tol >> n_reads >> n_bounds)) return 2;
        const float eval_tol = strtof(tol.c_str(), nullptr);  // ("inf": what operator>> does not read)
        CertState s(N, kmax, rmax, grow != 0, n_done, r_done, delta);
        FakeOps ops{s, eval_tol, std::vector<Read>((size_t)n_reads), std::vector<float>((size_t)n_bounds)};
        ops.spec_n_listed = std::min(kmax, N);
        ops.spec_delta = delta;
        for (Read& r : ops.reads)
            if (!(std::cin >> r.deviation >> r.need >> r.need_race)) return 2;
        for (float& b : ops.bounds)
            if (!(std::cin >> b)) return 2;
        printf("scenario %s\n", name.c_str());
        EvalState es(eval_tol);
        const int rc = m3pc::cert_resolve_eval(s, ops, es);
        m3pc_cert_record rec;
        m3pc::cert_record_fp32(N, &rec);  // (every field set, then every field the protocol owns overwritten)
        m3pc::cert_record(s, &rec);
        m3pc_eval_record erec = {-1.f, -1, -1, -1, -1};
        m3pc::cert_eval_record(es, &erec);
        printf("record rc=%d n_rescored=%d n_race=%d need_first=%d need_race_first=%d saturated=%d everything=%d certified=%d merges=%d "
               "delta=%.17g shift=%.17g reads_left=%d bounds_left=%d eval_bound=%.17g need_eval_first=%d n_eval=%d eval_rounds=%d "
               "eval_certified=%d\n",
               rc, rec.n_rescored, rec.n_race, rec.need_first, rec.need_race_first, rec.saturated, rec.everything, rec.certified, ops.merges,
               (double)rec.delta, (double)rec.shift, (int)(ops.reads.size() - ops.next), (int)(ops.bounds.size() - ops.next_bound),
               (double)erec.eval_bound, erec.need_eval_first, erec.n_eval, erec.eval_rounds, erec.eval_certified);
    }
    return 0;
}
