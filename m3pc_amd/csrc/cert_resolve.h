// The certified re-score's protocol (m3pc_amd/certificate.py:resolve) in plain C++: no HIP, standard headers only, so a host
// compiler builds it alone (tests/cert_resolve_host.cpp drives it with scripted certificates).  The device work comes from an
// ops object, as in certificate.py; m3pc_certified.hip has the two of the library: a single step (serial, eval, _begin / _end,
// _eval_begin / _eval_end) and a window of a lock-step batch.  cert_resolve_eval is the same loop with the eval_action certificate
// behind it (tests/cert_resolve_eval_host.cpp).
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

// The third certificate's state (m3pc_eval_record's fields, and the tolerance the ops' bound kernel takes).
struct EvalState {
    EvalState() {}
    explicit EvalState(float eval_tol_) : eval_tol(eval_tol_) {}
    float eval_tol = 0.f;
    float eval_bound = 0.f;   // the LAST bound read; 0 once every candidate has an fp32 score
    int need_eval_first = 0;  // what the FIRST bound asked for
    int n_eval = 0;           // score entries re-scored because this certificate asked
    int eval_rounds = 0;      // bounds the loop READ (a speculative launch that is discarded is not one)
    int eval_certified = 0;
};

// The loop with the eval_action certificate as a third one (m3pc_plan_step_certified_eval, _eval_end, a window of
// m3pc_plan_steps_certified_eval): cert_resolve, then the bound; what the bound asks for is re-scored, merged and selected, and
// every certificate is read again.  One more operation:
//   eval_read(n_listed, out8)      the eight statistics of the bound kernel behind the LAST merge + select, over the r_done race
//                                  entries and n_listed score entries of which n_done are re-scored, under delta as it stands
//                                  (blocks the host until they are there; the ops may hand back a launch they made in advance
//                                  when nothing it read has changed since)
// n_done strictly grows from turn to turn, so the loop ends.
template <class Ops>
int cert_resolve_eval(CertState& s, Ops& ops, EvalState& e) {
    for (;;) {
        if (int rc = cert_resolve(s, ops)) return rc;
        if (s.everything || s.n_done >= s.N) {  // the select ran on fp32 scores alone
            e.eval_bound = 0.f;
            e.eval_certified = 1;
            return 0;
        }
        float e8[8];
        const int n_listed = s.saturated ? s.n_done : (s.kmax < s.N ? s.kmax : s.N);  // (a window set's list is wholly re-scored)
        if (int rc = ops.eval_read(n_listed, e8)) return rc;
        const int need_eval = (int)e8[1];
        if (++e.eval_rounds == 1) e.need_eval_first = need_eval;
        e.eval_bound = e8[0];
        if (need_eval <= s.n_done) {
            e.eval_certified = 1;
            return 0;
        }
        if (need_eval <= n_listed) {  // score entries [n_done, need_eval), merge + select again, every certificate read again
            if (int rc = ops.extend(s.n_done, need_eval)) return rc;
            e.n_eval += need_eval - s.n_done;
            s.n_done = need_eval;
            if (int rc = ops.merge_select()) return rc;
        } else {  // the list cannot reach the tolerance: every candidate in fp32
            if (int rc = ops.window_set(s.N, true)) return rc;
            s.everything = true;
        }
    }
}
// m3pc_eval_record from the state the loop left (a template, as cert_record)
template <class Rec>
void cert_eval_record(const EvalState& e, Rec* erec) {
    erec->eval_bound = e.eval_bound;
    erec->need_eval_first = e.need_eval_first;
    erec->n_eval = e.n_eval;
    erec->eval_rounds = e.eval_rounds;
    erec->eval_certified = e.eval_certified;
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
