// The certified re-score's protocol (m3pc_amd/certificate.py:resolve) in plain C++: no HIP, standard headers only, so a host
// compiler builds it alone (tests/cert_resolve_host.cpp drives it with scripted certificates).  The device work comes from an
// ops object, as in certificate.py; m3pc_certified.hip has the two of the library: a single step (serial, eval, _begin / _end)
// and a window of a lock-step batch.
#pragma once
#include <string.h>

namespace m3pc {

// One step's (one window's) re-score as the protocol sees it.  A first pass has been enqueued already: the n_done best
// candidates by low-precision score and the r_done best by race key re-scored in fp32, merged, selected.
struct CertState {
    CertState() {}
    CertState(int N_, int kmax_, int rmax_, bool grow_delta_, int n_done_, int r_done_, double delta_)
        : N(N_), kmax(kmax_), rmax(rmax_), grow_delta(grow_delta_), n_done(n_done_), r_done(r_done_), delta(delta_) {}
    int N = 0, kmax = 0, rmax = 0;  // candidates; score / race entries the lists hold
    bool grow_delta = false;        // raise delta to 1.5 x the deviation the re-scored set shows
    int n_done = 0, r_done = 0;     // score / race entries re-scored in fp32
    double delta = 0.0;             // (1.5 x a float deviation needs 25 bits: kept as the double the Python protocol keeps)
    bool saturated = false, everything = false;  // window set taken / fp32 scores for every candidate: both outlive a call
    int need = 0, need_race = 0;    // what the certificates read last ask for
    bool read_any = false;          // need_first / need_race_first are set: by the very first read only
    int need_first = 0, need_race_first = 0;
    float stats[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // the last read: shift, deviation, need, margin, seq, need_race, K*, its threshold
};

// The loop.  Every operation returns an int; non-zero ends the loop with that code.
//   read(four_only, out8)          the statistics of the LAST merge (blocks the host until they are there); four_only: that
//                                  merge had no race entries and wrote four statistics
//   extend(lo, hi)                 fp32 re-score of the entries [lo, hi) of the score list
//   extend_race(lo, hi)            fp32 re-score of the entries [lo, hi) of the race list
//   window_set(need, everything)   the lists are too short: re-score the `need` best candidates by score (or every candidate:
//                                  beyond the list capacity, or when the race list is exhausted), leave merge + select
//                                  enqueued and set n_done
//   merge_select()                 merge + select again over the n_done + r_done re-scored entries, under delta
// Read the certificates; raise delta when the re-scored set deviates by more than it allows (then merge again: both counts
// depend on delta); re-score what a certificate asks for; stop when both are satisfied or every candidate has been scored in fp32.
template <class Ops>
int cert_resolve(CertState& s, Ops& ops) {
    for (;;) {
        if (int rc = ops.read(s.everything || s.rmax == 0, s.stats)) return rc;
        s.need = (int)s.stats[2];
        s.need_race = (int)s.stats[5];
        if (!s.read_any) {
            s.read_any = true;
            s.need_first = s.need;
            s.need_race_first = s.need_race;
        }
        bool redo = false;
        if (s.grow_delta && 1.5 * (double)s.stats[1] > s.delta && !s.everything) {
            s.delta = 1.5 * (double)s.stats[1];
            redo = s.n_done < s.N;
        }
        if (s.everything || s.n_done >= s.N) return 0;
        if (!redo) {
            if (s.need > s.n_done && s.saturated) {  // the window set's certificate still asks for more: every candidate in fp32
                if (int rc = ops.window_set(s.N, true)) return rc;
                s.everything = true;
                continue;
            }
            if (s.need > s.n_done) {
                if (s.need <= s.kmax) {
                    if (int rc = ops.extend(s.n_done, s.need)) return rc;
                    s.n_done = s.need;
                    redo = true;
                } else {
                    if (int rc = ops.window_set(s.need, false)) return rc;
                    s.saturated = true;
                    s.everything = s.n_done >= s.N;
                    continue;
                }
            }
            if (s.need_race > s.r_done) {
                if (s.need_race <= s.rmax) {
                    if (int rc = ops.extend_race(s.r_done, s.need_race)) return rc;
                    s.r_done = s.need_race;
                    redo = true;
                } else {  // more racers than the race list holds: every candidate in fp32
                    if (int rc = ops.window_set(s.N, true)) return rc;
                    s.saturated = s.everything = true;
                    continue;
                }
            }
        }
        if (!redo) return 0;
        if (int rc = ops.merge_select()) return rc;
    }
}

// The step's record (m3pc_cert_record; a template so that this header needs no other) from the state the loop left.  `rounds`
// stays with whoever counts the merges.  certified: the loop ended on satisfied certificates or on fp32 scores for every
// candidate -- it cannot end otherwise, the record says so for callers and tests.
template <class Rec>
void cert_record(const CertState& s, Rec* rec) {
    rec->n_rescored = s.n_done;
    rec->n_race = s.r_done;
    rec->need_first = s.need_first;
    rec->need_race_first = s.need_race_first;
    rec->saturated = s.saturated;
    rec->everything = s.everything;
    rec->certified = s.everything || s.n_done >= s.N || (s.need <= s.n_done && s.need_race <= s.r_done);
    rec->delta = (float)s.delta;
    rec->shift = s.stats[0];
    rec->deviation = s.stats[1];
    rec->margin = s.stats[3];
}
// the record of a step whose candidate pass ran in fp32: nothing to certify
template <class Rec>
void cert_record_fp32(int N, Rec* rec) {
    memset(rec, 0, sizeof(*rec));
    rec->n_rescored = N;
    rec->everything = rec->certified = 1;
}

// max(factor x the largest deviation from the median, 1e-6 x the scores' scale, 1e-30): the host arithmetic of
// HipPlanner._calibrate (doubles of the device's floats), rounded once to the float the ABI carries
inline float cert_delta(float factor, float deviation, float f_max) {
    double d = (double)factor * (double)deviation;
    if (1e-6 * (double)f_max > d) d = 1e-6 * (double)f_max;
    if (1e-30 > d) d = 1e-30;
    return (float)d;
}

}  // namespace m3pc
