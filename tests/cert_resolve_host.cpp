// The protocol loop of m3pc_amd/csrc/cert_resolve.h driven without a device: scripted certificates in, the trace of ops calls
// and the final record out (tests/test_cert_resolve_cpu.py compares both with m3pc_amd/certificate.py:resolve).
//
// stdin, per scenario:   name N kmax rmax n_done r_done delta grow n_reads n_entries
//                        n_reads lines            deviation need need_race
//                        n_entries - 1 numbers    ext   (before entry i >= 1: ext > n_done scores the entries [n_done, ext) and
//                                                 merges, as a turn of the eval certificate does; then the loop is entered again
//                                                 on the SAME state)
// Read i (from 0) carries shift = (i + 1) / 8 and margin = (i + 1) / 16, so the record shows which read came last.
#include <stdio.h>

#include <algorithm>
#include <iostream>
#include <string>
#include <vector>

#include "cert_resolve.h"
#include "m3pc_hip.h"

using m3pc::CertState;

struct Read {
    float deviation;
    int need, need_race;
};

struct FakeOps {
    CertState& s;
    std::vector<Read> reads;
    size_t next = 0;
    int read(bool four_only, float* out8) {
        printf("read %d\n", (int)four_only);
        if (next == reads.size()) return 99;  // the script is exhausted: the loop asked for more than the scenario foresaw
        const Read& r = reads[next++];
        const float v[8] = {(float)next / 8.f, r.deviation, (float)r.need, (float)next / 16.f, 0.f, (float)r.need_race, 0.f, 0.f};
        std::copy(v, v + 8, out8);
        return 0;
    }
    int extend(int lo, int hi) { return printf("extend %d %d\n", lo, hi), 0; }
    int extend_race(int lo, int hi) { return printf("extend_race %d %d\n", lo, hi), 0; }
    int window_set(int need, bool everything) {
        printf("window_set %d %d %.17g\n", need, (int)everything, s.delta);
        s.n_done = everything ? s.N : std::min(need, s.N);
        return 0;
    }
    int merge_select() { return printf("merge_select %d %d %.17g\n", s.n_done, s.r_done, s.delta), 0; }
};

int main() {
    std::string name;
    while (std::cin >> name) {
        int N, kmax, rmax, n_done, r_done, grow, n_reads, n_entries;
        double delta;
        if (!(std::cin >> N >> kmax >> rmax >> n_done >> r_done >> delta >> grow >> n_reads >> n_entries)) return 2;
        CertState s(N, kmax, rmax, grow != 0, n_done, r_done, delta);
        FakeOps ops{s, std::vector<Read>((size_t)n_reads)};
        for (Read& r : ops.reads)
            if (!(std::cin >> r.deviation >> r.need >> r.need_race)) return 2;
        printf("scenario %s\n", name.c_str());
        int rc = 0;
        for (int e = 0; e < n_entries && rc == 0; ++e) {
            if (e > 0) {
                int ext;
                if (!(std::cin >> ext)) return 2;
                if (ext > s.n_done) {
                    ops.extend(s.n_done, ext);
                    s.n_done = ext;
                    ops.merge_select();
                }
                printf("enter\n");
            }
            rc = m3pc::cert_resolve(s, ops);
        }
        m3pc_cert_record rec;
        m3pc::cert_record_fp32(N, &rec);  // (every field set, then every field the protocol owns overwritten)
        m3pc::cert_record(s, &rec);
        printf("record rc=%d n_rescored=%d n_race=%d need_first=%d need_race_first=%d saturated=%d everything=%d certified=%d rounds=%d "
               "delta=%.17g shift=%.17g deviation=%.17g margin=%.17g reads_left=%d\n",
               rc, rec.n_rescored, rec.n_race, rec.need_first, rec.need_race_first, rec.saturated, rec.everything, rec.certified, rec.rounds,
               (double)rec.delta, (double)rec.shift, (double)rec.deviation, (double)rec.margin, (int)(ops.reads.size() - ops.next));
    }
    m3pc_cert_record fp32;
    m3pc::cert_record_fp32(625, &fp32);
    printf("fp32 n_rescored=%d everything=%d certified=%d saturated=%d rounds=%d delta=%.17g\n", fp32.n_rescored, fp32.everything,
           fp32.certified, fp32.saturated, fp32.rounds, (double)fp32.delta);
    printf("cert_delta %.17g %.17g %.17g\n", (double)m3pc::cert_delta(2.f, 0.125f, 8.f), (double)m3pc::cert_delta(2.f, 0.f, 8.f),
           (double)m3pc::cert_delta(2.f, 0.f, 0.f));
    return 0;
}
