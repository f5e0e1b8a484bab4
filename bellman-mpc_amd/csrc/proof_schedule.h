// The enqueue schedule of one proof's multiexps (prover.hip, compute_msms) as data: which of the 8
// multiexps are large, where each one's sort, accumulation and reduction tail go, what a sort
// takes its entries from, where H is enqueued, and the order of the host's enqueues.  Plain host
// C++, computed before anything is enqueued: the prover's executor walks the steps, and the host
// test (bh_selftest_proof_schedule, tests/test_proof_schedule_cpu.py) reads this one function.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bh {

constexpr size_t SMALL_JOB = 4096;  // run whole on a side stream (latency-bound)

// Streams, all ordered after whatever ran before on the main one:
//   main    : the bucket accumulations back to back (VALU-bound critical path);
//   H       : the H pipeline (after the first accumulation, or first when distributed);
//   sort    : density maps, then every multiexp's sort (memory-bound, runs ahead);
//   small   : the small (public-input) multiexps, whole;
//   lane 3  : the third accumulation lane;
//   tail k  : the reduction tail of the q-th large multiexp, k = q % 5.
// Each multiexp has its own workspace, so the only dependencies are the steps' events.
enum SchedStream : int8_t { SCHED_MAIN = 0, SCHED_SMALL, SCHED_SORT, SCHED_H, SCHED_LANE3, SCHED_TAIL0 };
constexpr int SCHED_TAIL_STREAMS = 5;
constexpr int SCHED_STREAMS = SCHED_TAIL0 + SCHED_TAIL_STREAMS;

// What multiexp j's sort can take from multiexp i's (SchedIn::rel[i][j]).
// SAME: two multiexps with the same scalars, density map, range and digit geometry (b_g1_aux and
// b_g2_aux: prover.rs:282-307 both use the aux assignment under b_aux_density) have identical
// sorted entries, so the second one copies the first one's instead of sorting.
// DERIVABLE: ... and one over a sparser density map (a_aux, b_aux under l's dense one) compacts it.
enum SchedRel : uint8_t { SCHED_REL_NONE = 0, SCHED_REL_SAME, SCHED_REL_DERIVABLE };
enum SchedSortKind : int8_t { SCHED_SORT_REAL = 0, SCHED_SORT_COPY, SCHED_SORT_DERIVE };

enum SchedOp : int8_t {
  SCHED_OP_H = 0,     // the H pipeline
  SCHED_OP_SORT,      // digit sort (or copy / compaction of another's) + its max-span words
  SCHED_OP_ACC,       // bucket accumulation
  SCHED_OP_TAIL,      // reduction tail
  SCHED_OP_MARK_ACC0, // host timestamp: the first accumulation(s) are enqueued
  SCHED_OP_MARK_SORTS,// host timestamp: the sorts are enqueued
  SCHED_OP_HANDOFF,   // everything but the large tails is enqueued: the per-stream done events,
                      // then a pipelined batch lane hands the streams to the next proof
};

struct SchedStep {
  int8_t op, job = -1, stream = SCHED_MAIN;
  int8_t kind = SCHED_SORT_REAL, src = -1;  // sort: what it is and whose entries it takes
  int8_t pre = 0;          // sort: runs ahead of the first accumulation
  int8_t wait_h = 0;       // sort: behind a wait on the H-done event (distributed H)
  int8_t wait_sorted = -1; // the first accumulation: also waits for this multiexp's sort (wait_j)
  int8_t slot = -1;        // tail: its position among the large multiexps (its done event)
};

struct SchedJob {
  size_t len = 0;   // this shard's scalars, hi - lo
  size_t used = 0;  // density-set scalars of the whole query (the lane balance weighs by it)
  int W = 0;        // digit windows
  bool is_h = false, g2 = false;
};

struct SchedIn {
  SchedJob job[8];
  uint8_t rel[8][8] = {};  // SchedRel of [i][j]: what j's sort can take from i's
  bool serial = false;     // one stream (per-kernel profiling)
  bool borrowed_streams = false;  // a pipelined batch lane: the streams are its primary's
  bool cu_masked = false;  // the tail streams are CU-masked
  bool host_in = false;    // the public-input multiexps run on the host thread
  bool uploading = false;  // the witness is still uploading (bh_prove)
  bool distributed = false;// H is distributed over the ranks
};

constexpr int SCHED_MAX_STEPS = 32;  // 1 H + 8 x (sort, accumulation, tail) + 3 marks

struct ProofSchedule {
  int big[8], nbig = 0, small[8], nsmall = 0;
  bool h_first = false;    // H is the first thing enqueued (else just before h's own accumulation)
  bool first_own = false;  // the first accumulation has the small-multiexp stream to itself
  bool multi_lane = false; // three accumulation lanes
  int wait_j = -1;         // the sort the first accumulation's stream waits for
  SchedStep steps[SCHED_MAX_STEPS];
  int nsteps = 0;
};

// proof_schedule()'s working state: the schedule so far, and what its later phases read of the
// earlier ones.  The phases run in the order of the host's enqueues.
struct ScheduleBuilder {
  const SchedIn& in;
  ProofSchedule P;
  bool own_sort[8] = {false};  // the multiexp's real or derived sort is among the steps so far
  int8_t acc_stream[8];        // the stream of the q-th large multiexp's accumulation
  bool h_late = false;         // H just before h's own accumulation
  int pre_sorts = 0, q_first = 1;

  SchedStep& push(SchedOp op, int job, int stream) {
    SchedStep& s = P.steps[P.nsteps++];
    s = SchedStep{};
    s.op = op; s.job = (int8_t)job; s.stream = (int8_t)stream;
    return s;
  }
  // The sorts, walked in the order they are enqueued: a multiexp is a usable source only once its
  // own real or derived sort is ahead (a copy is not: it may take it from the same source).
  SchedStep& sort_step(int j, int stream) {
    SchedStep& s = push(SCHED_OP_SORT, j, stream);
    for (int i = 0; i < 8 && s.src < 0; i++)
      if (i != j && own_sort[i] && in.rel[i][j] == SCHED_REL_SAME) { s.src = (int8_t)i; s.kind = SCHED_SORT_COPY; }
    // a fully dense sort over the same scalars and digits to compact from
    for (int i = 0; i < 8 && s.src < 0; i++)
      if (i != j && own_sort[i] && in.rel[i][j] == SCHED_REL_DERIVABLE) { s.src = (int8_t)i; s.kind = SCHED_SORT_DERIVE; }
    own_sort[j] = s.kind != SCHED_SORT_COPY;  // a derived sort is one of its own from here on (copies may take it)
    return s;
  }
  // h's digit sort reads the H block's output: on a replicated H it runs on the H stream right
  // behind it, so the sort stream never waits for H (a pipelined batch's next proof queues its
  // density maps and sorts there, behind this proof's); distributed H (CU-masked stream) keeps it
  // on the sort stream after an event wait
  void sort_h_or(int j, bool pre) {
    SchedStep& s = sort_step(j, in.job[j].is_h && !in.distributed ? SCHED_H : SCHED_SORT);
    s.wait_h = in.job[j].is_h && in.distributed;
    s.pre = pre;
  }

  // which multiexps are large, and the start-up: H, the sorts that run ahead, the first accumulations
  void start_up() {
    const SchedJob* jobs = in.job;
    for (int j = 0; j < 8; j++) {
      const size_t n = jobs[j].len;
      if (!n || (in.host_in && j >= 5)) continue;
      if (n < SMALL_JOB && !jobs[j].is_h) P.small[P.nsmall++] = j;
      else P.big[P.nbig++] = j;
    }
    const int nbig = P.nbig;
    const int* big = P.big;
    // Large ones: sorts run ahead on the sort stream, accumulations back to back on the main stream,
    // each reduction tail on a stream of its own (the tails are latency-bound chains of point
    // additions: several run side by side at little cost, and none waits behind another).
    int h_pos = nbig;
    for (int q = 0; q < nbig; q++)
      if (jobs[big[q]].is_h) h_pos = q;
    // (Tried and removed: the last multiexp accumulated and reduced as two bucket halves so the
    // lower half's reduction runs beside the upper half's accumulation, +0.8 ms per 2^22 proof,
    // profiles/r03_ab_last_halves.txt; fewer rounds for the last accumulation, within noise.)
    // H placement.  A resident witness enqueues H first, running beside everything: since the G2
    // accumulation keeps ZZ/ZZZ in LDS (268 registers, msm_impl.cuh accumulate_lds) H's NTT passes
    // co-reside with it (same-box A/B at 2^22: 55.1-55.3 ms per proof against 57.4-58.2 with H after
    // the first accumulation, profiles/r04_ab_hmode_g2.txt).  Other placements were measured and
    // removed: H enqueued after the first accumulation's launch, between the first sorts and the first
    // accumulation, from a helper host thread, or held on the device until the first sort is done
    // (N = 8 rehearsal within 0.1 ms or slower, profiles/r03_ab_hmode_N8.txt, r03_ab_hmode_more_N8.txt,
    // r05_ab_sched_knobs_N1_2_8.txt).  From host buffers (bh_prove) the uploading thread enqueues H
    // vector by vector behind each upload (on_vector); here only h's own sort and accumulation wait on
    // the host for that enqueue, so they are enqueued last.
    h_late = in.uploading;
    // Host enqueue order follows the critical path: the first two sorts (a sort running beside
    // a whole-GPU accumulation only gets CUs as its workgroups retire, so the second one would
    // not be ready when the first accumulation ends), the first accumulation, H, the remaining
    // sorts (h's after H), every accumulation, the small multiexps, then the tails.
    // Sort order = accumulation order (b_g2_aux sorted, b_g1_aux copied, l sorted, a_aux
    // compacted from l, h): putting l first so that b_g2_aux could be compacted from it would
    // lengthen the start-up (measured +2 ms at 2^22), so only later sorts are derived.
    // every sort up to those of the first two accumulations runs ahead of the first accumulation
    pre_sorts = nbig == 0 ? 0 : nbig > 1 && h_pos != 1 ? 2 : 1;
    bool h_in_pre = false;
    for (int r = 0; r < pre_sorts; r++) h_in_pre = h_in_pre || jobs[big[r]].is_h;
    if (h_in_pre) h_late = false;  // h's own sort is among the first: H first
    P.h_first = !h_late;
    if (!h_late) push(SCHED_OP_H, -1, SCHED_H);
    for (int r = 0; r < pre_sorts; r++) sort_h_or(big[r], true);
    // The first accumulation (G2: 268 registers, one wave per SIMD) runs on the small-multiexp
    // stream (idle when the public-input multiexps are on the host), so the G1 accumulations start
    // beside it instead of after it: same-box A/B at 2^22 54.66-55.17 against 55.01-55.45 ms
    // (profiles/r04_ab_first_acc_stream.txt).
    P.first_own = P.nsmall == 0 && !in.serial;
    for (int q = 0; q < 8; q++) acc_stream[q] = -1;
    if (nbig > 0) {
      // wait for the last pre-sort that is a real sort: a trailing copy of another multiexp's
      // entries (b_g1_aux from b_g2_aux) is ~0.15 ms of blits that can run beside the accumulation
      P.wait_j = big[0];
      for (int r = 0; r < pre_sorts; r++)
        if (own_sort[big[r]]) P.wait_j = big[r];
      acc_stream[0] = P.first_own ? SCHED_SMALL : SCHED_MAIN;
      push(SCHED_OP_ACC, big[0], acc_stream[0]).wait_sorted = (int8_t)P.wait_j;
    }
    // With the first accumulation on its own stream, the second one (G1: b_g1_aux, whose sorted
    // entries are a copy among the first sorts) is enqueued right behind it, before the remaining
    // sorts: those are ~20-40 host enqueues (~0.7 ms per rank at N = 8 in the round-5 kernel
    // trace, 1.6 ms at N = 2), during which the G2 accumulation ran alone on its one wave per SIMD.
    // (only where its sort is among the pre-sorts, enqueued above)
    if (nbig > 1 && !jobs[big[1]].is_h && P.first_own && pre_sorts > 1) {
      acc_stream[1] = SCHED_MAIN;
      push(SCHED_OP_ACC, big[1], SCHED_MAIN);
      q_first = 2;
    }
    push(SCHED_OP_MARK_ACC0, -1, SCHED_MAIN);
  }

  // the remaining sorts, every other accumulation on its lane, then the small multiexps
  void sorts_and_lanes() {
    const SchedJob* jobs = in.job;
    const int nbig = P.nbig;
    const int* big = P.big;
    for (int r = pre_sorts; r < nbig; r++) {
      if (h_late && jobs[big[r]].is_h) continue;  // behind H, enqueued below
      sort_h_or(big[r], false);
    }
    push(SCHED_OP_MARK_SORTS, -1, SCHED_MAIN);
    // Accumulation lanes: the accumulations after the first two go to whichever of three accumulation
    // streams (the first one's, the main one, lane 3) has the least queued work (mixed additions, a G2
    // one weighted 2.75x).  Consecutive accumulations on one stream are separated by a barrier (the
    // next kernel dispatches only once the last block of the previous one is done: ~0.12 ms between
    // them in the round-5 traces), and in that moment other streams' pending kernels take the freed
    // slots (round-5 drop-in trace: 1.4 and 2.9 ms of main-stream idle before a_aux and h).  Two lanes
    // (round 5): rehearsal N = 8 9.85-9.92 against 10.05-10.23 ms per rank (profiles/r05_ab_acc_lanes.txt);
    // with the G2 accumulation holding one lane for most of the proof, the G1 ones still ran back to
    // back on the other, so round 6 adds a third: the 2^22 bench 54.4-54.6 against 54.8-55.0 ms, bh_prove
    // 58.7-58.9 against 59.5-59.7, N = 2 30.4 against 30.8-31.2 ms per rank, N = 1 and 8 within noise
    // (profiles/r06_ab_acc_lanes3.txt).
    P.multi_lane = P.first_own && !in.borrowed_streams && nbig > 2;
    auto acc_cost = [&](int j) {
      const double e = (double)jobs[j].used * (double)(jobs[j].W ? jobs[j].W : 1);
      return jobs[j].g2 ? 2.75 * e : e;
    };
    double lane_load[3] = {nbig > 0 ? acc_cost(big[0]) : 0.0, 0.0, 0.0};  // [0] small, [1] main, [2] lane 3
    for (int q = 1; q < q_first; q++) lane_load[1] += acc_cost(big[q]);
    bool h_done = !h_late;
    for (int q = q_first; q < nbig; q++) {
      if (!h_done && jobs[big[q]].is_h) {
        push(SCHED_OP_H, -1, SCHED_H);
        sort_h_or(big[q], false);
        h_done = true;
      }
      acc_stream[q] = SCHED_MAIN;
      if (P.multi_lane) {
        int l = lane_load[0] < lane_load[1] ? 0 : 1;
        if (lane_load[2] < lane_load[l]) l = 2;
        lane_load[l] += acc_cost(big[q]);
        acc_stream[q] = l == 0 ? SCHED_SMALL : l == 1 ? SCHED_MAIN : SCHED_LANE3;
      }
      push(SCHED_OP_ACC, big[q], acc_stream[q]);
    }
    if (!h_done) push(SCHED_OP_H, -1, SCHED_H);  // (no large h job: H still runs)
    // the small multiexps run whole on their own stream, after the density maps
    for (int i = 0; i < P.nsmall; i++) {
      sort_step(P.small[i], SCHED_SMALL);
      push(SCHED_OP_ACC, P.small[i], SCHED_SMALL);
      push(SCHED_OP_TAIL, P.small[i], SCHED_SMALL);
    }
    push(SCHED_OP_HANDOFF, -1, SCHED_MAIN);
  }

  // the large multiexps' reduction tails
  void tails() {
    const int nbig = P.nbig;
    int8_t tail[8];
    for (int q = 0; q < 8; q++) tail[q] = (int8_t)(SCHED_TAIL0 + q % SCHED_TAIL_STREAMS);
    // The last multiexp's reduction tail runs when every accumulation is done, alone at the end of
    // the critical path: on the CU-masked tail streams (a quarter of the CUs) its 2^19-bucket
    // reduction needed two rounds of resident blocks.  So it runs on the
    // small-multiexp stream (high priority, every CU), with its bucket reduction shaped for one round
    // of the whole GPU (not on a pipelined batch lane, whose next proof's first accumulation would
    // queue behind it).
    const bool last_full = !in.serial && !in.borrowed_streams && in.cu_masked;
    // The last tail right behind its own accumulation, on that lane (every CU): with three lanes
    // (round 6) the first accumulation's stream may still be running the G2 tail below, which held
    // the last tail back 0.9 ms at N = 8 (profiles/r06_n8_rank0_timeline.txt, second trace).
    if (last_full && nbig > 0 && P.nsmall == 0)
      tail[nbig - 1] = P.multi_lane ? acc_stream[nbig - 1] : (int8_t)SCHED_SMALL;
    // The G2 multiexp's reduction tail (continuation fold + reduction of G2 buckets, each addition
    // ~3x a G1 one) on the first accumulation's stream, every CU, right behind the G2 accumulation,
    // rather than on a quarter-CU tail stream: with three accumulation lanes the G1 accumulations end
    // earlier and at N = 8 that latency-bound tail (2.9 + 1.6 + 0.8 ms on 64 CUs) became the rank's
    // critical path (profiles/r06_n8_rank0_timeline.txt).  Same-box A/B: the 2^22 bench 53.9-54.0 against 54.3-54.8
    // ms, bh_prove 57.9-58.2 against 58.4-58.9, rehearsal N = 1 / 2 / 8 at or below the base
    // (profiles/r06_ab_g2_tail.txt).  (On a pipelined batch lane the streams are shared: tail streams.)
    // (only where no later accumulation queued on that stream: the tail would wait for it)
    if (!in.serial && !in.borrowed_streams)
      for (int q = 0; q + 1 < nbig; q++) {
        if (!in.job[P.big[q]].g2) continue;
        bool later = false;
        for (int r = q + 1; r < nbig; r++) later = later || acc_stream[r] == acc_stream[q];
        if (!later) tail[q] = acc_stream[q];
      }
    for (int q = 0; q < nbig; q++) push(SCHED_OP_TAIL, P.big[q], tail[q]).slot = (int8_t)q;
  }
};

inline ProofSchedule proof_schedule(const SchedIn& in) {
  ScheduleBuilder b{in};
  b.start_up();
  b.sorts_and_lanes();
  b.tails();
  if (in.serial)  // one stream
    for (int i = 0; i < b.P.nsteps; i++) b.P.steps[i].stream = SCHED_MAIN;
  return b.P;
}

}  // namespace bh
