// Detections of one frame associated with the tracks of the frames before it, for the image library (image.hip):
//  * track_update_f32 — a greedy IoU tracker with an optional constant-velocity prediction as one launch of one
//    workgroup. The tracker's state lives in device buffers that the kernel updates in place, so each replay of a
//    captured graph is the next frame. Thread t owns track slot t; thread r reads detection row r; the candidates are
//    ordered by score (the rank count of merge_detections_f32) and passed one per barrier, each taking the untaken
//    live track of its label whose predicted box it overlaps most (a workgroup arg-max); what stays unmatched starts
//    tracks in the free slots (two ballot scans).
// Included by image.hip alone, after image_detect.h (box_overlap, DT, DW, MMAX).
#pragma once
#include <hip/hip_runtime.h>

#include "image_detect.h"

namespace {
constexpr int TMAX = 1024;
static_assert(TMAX == DT && MMAX == DT, "one thread per track slot and per detection row");

// One frame: count [1] (clamped to 0..N here), scores / labels / boxes [N](x4) as detections_f32 and
// merge_detections_f32 write them; row r is a candidate when r < count and scores[r] > 0 (a NaN is not).
// The state, T slots: t_boxes / t_vel [T][4], t_labels / t_ids / t_hits / t_misses [T] (ids == 0: a free slot, all of
// it zero), next_id [1], dropped [1].
//   predict  a live track's box + vel (motion = 1) or its box (motion = 0)
//   match    candidates by score descending (ties: the lower row); each takes the live, untaken track of its label
//            with the largest IoU of the predicted box, when that exceeds mt (ties: the lowest slot)
//   matched  vel += gain * ((box - old) - vel) (motion = 1), box = the detection's, hits + 1, misses = 0
//   others   misses + 1; past max_age the slot is zeroed, else box += vel (motion = 1)
//   births   unmatched candidates with score > bt, in that order, into the free slots ascending (those freed just now
//            included): ids from next_id, hits 1; without a slot a candidate adds 1 to dropped
// track_id / track_hits [N], by input row: the id and hits of the row's track after the update, 0 for every other row.
// Every trip count of a loop that holds a barrier (the number of candidates) and every pivot's outcome is read from
// LDS by all threads. Static LDS: 12 tables of 1024 words and three of 2 x 16 = 48.4 KB.
__global__ __launch_bounds__(DT) void track_update_f32(const int* __restrict__ count, const float* __restrict__ scores,
                                                        const int* __restrict__ labels, const float* __restrict__ boxes,
                                                        int N, float* __restrict__ t_boxes, float* __restrict__ t_vel,
                                                        int* __restrict__ t_labels, int* __restrict__ t_ids,
                                                        int* __restrict__ t_hits, int* __restrict__ t_misses,
                                                        int* __restrict__ next_id, int* __restrict__ dropped, int T,
                                                        float mt, int max_age, float bt, int motion, float gain,
                                                        int* __restrict__ track_id, int* __restrict__ track_hits) {
  __shared__ float s_score[MMAX];                               // by row: a candidate's score, 0 for any other row
  __shared__ float q_score[MMAX];                               // by rank among the candidates
  __shared__ int q_label[MMAX], q_row[MMAX], q_id[MMAX], q_hits[MMAX];
  __shared__ float q_box[MMAX * 4];
  __shared__ int s_free[TMAX], s_born[TMAX];                    // the free slots ascending; the rank born into a slot
  __shared__ float w_iou[2][DW];                                // per wave, double-buffered: one barrier per candidate
  __shared__ int w_slot[2][DW];
  __shared__ int s_wave[2][DW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int first_id = next_id[0];                              // read before the first barrier, written after the last
  const int n = min(max(count[0], 0), N);
  float si = 0.f;
  if (tid < n) {
    const float s = scores[tid];
    si = s > 0.f ? s : 0.f;
  }
  if (tid < N) s_score[tid] = si;
  s_born[tid] = -1;
  // slot tid's track, in registers from here to the end
  const bool mine = tid < T;
  float box[4] = {0.f, 0.f, 0.f, 0.f}, vel[4] = {0.f, 0.f, 0.f, 0.f}, pred[4];
  int lab = 0, id = 0, hits = 0, misses = 0;
  if (mine) {
#pragma unroll
    for (int c = 0; c < 4; ++c) box[c] = t_boxes[tid * 4 + c], vel[c] = t_vel[tid * 4 + c];
    lab = t_labels[tid], id = t_ids[tid], hits = t_hits[tid], misses = t_misses[tid];
  }
  const bool live = id != 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) pred[c] = motion ? box[c] + vel[c] : box[c];
  __syncthreads();
  // the order: thread i counts the candidates that precede row i, and every thread the candidates
  const bool cand = si > 0.f;
  int rank = 0, ncand = 0;
  for (int j = 0; j < N; ++j) {
    const float sj = s_score[j];
    const bool cj = sj > 0.f;
    ncand += cj;
    rank += cj && (sj > si || (sj == si && j < tid));
  }
  if (cand) {
    q_score[rank] = si;
    q_label[rank] = labels[tid];
    q_row[rank] = tid;
    q_id[rank] = 0;
    q_hits[rank] = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) q_box[rank * 4 + c] = boxes[tid * 4 + c];
  }
  __syncthreads();
  // the greedy pass: candidate p against every slot at once. Each wave reduces its 64 slots, lane 0 leaves the wave's
  // best in w_*[p & 1], and after the barrier every thread reads the waves' entries and finds the same winner. The
  // entries of p are overwritten in iteration p + 2, which a thread enters only after the barrier of p + 1, and that
  // barrier every thread reaches after its reads of p.
  const int nw = (T + 63) >> 6;
  bool taken = false;
  for (int p = 0; p < ncand; ++p) {
    const int buf = p & 1;
    float ov = -1.f;
    if (live && !taken && lab == q_label[p]) {
      const float o = box_overlap(q_box + p * 4, pred, 1);
      if (o > mt) ov = o;
    }
    if (wave < nw) {
      float best = ov;
      int slot = tid;
      if (__ballot(ov >= 0.f)) {  // the same in every lane of the wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const float ob = __shfl_xor(best, o);
          const int os = __shfl_xor(slot, o);
          if (ob > best || (ob == best && os < slot)) best = ob, slot = os;
        }
      }
      if (lane == 0) w_iou[buf][wave] = best, w_slot[buf][wave] = slot;
    }
    __syncthreads();
    float best = -1.f;
    int slot = -1;
    for (int w = 0; w < nw; ++w) {
      const float o = w_iou[buf][w];
      if (o > best) best = o, slot = w_slot[buf][w];  // strictly: the lower wave keeps a tie
    }
    if (slot == tid) {  // a winner overlaps by more than mt >= 0, so slot stays -1 when no track qualifies
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float b = q_box[p * 4 + c];
        if (motion) vel[c] += gain * ((b - box[c]) - vel[c]);
        box[c] = b;
      }
      hits += 1;
      misses = 0;
      taken = true;
      q_id[p] = id;
      q_hits[p] = hits;
    }
  }
  // the live tracks nothing took
  bool freed = mine && !live;
  if (live && !taken) {
    misses += 1;
    if (misses > max_age) {
      freed = true;
      lab = id = hits = misses = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) box[c] = vel[c] = 0.f;
    } else if (motion) {
#pragma unroll
      for (int c = 0; c < 4; ++c) box[c] += vel[c];
    }
  }
  __syncthreads();  // q_id of the matched candidates
  // births: thread k as candidate k asks for a slot, thread t as slot t offers one
  const bool want = tid < ncand && q_id[tid] == 0 && q_score[tid] > bt;
  const unsigned long long wmask = __ballot(want), fmask = __ballot(freed);
  if (lane == 0) s_wave[0][wave] = __popcll(wmask), s_wave[1][wave] = __popcll(fmask);
  __syncthreads();
  int bi = 0, nb = 0, fi = 0, nf = 0;
  for (int w = 0; w < DW; ++w) {
    bi += w < wave ? s_wave[0][w] : 0;
    nb += s_wave[0][w];
    fi += w < wave ? s_wave[1][w] : 0;
    nf += s_wave[1][w];
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  bi += __popcll(wmask & below);
  fi += __popcll(fmask & below);
  if (freed) s_free[fi] = tid;
  __syncthreads();
  if (want && bi < nf) {
    s_born[s_free[bi]] = tid;
    q_id[tid] = first_id + bi;
    q_hits[tid] = 1;
  }
  __syncthreads();
  if (mine) {
    const int k = s_born[tid];
    if (k >= 0) {
      lab = q_label[k], id = q_id[k], hits = 1, misses = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) box[c] = q_box[k * 4 + c], vel[c] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) t_boxes[tid * 4 + c] = box[c], t_vel[tid * 4 + c] = vel[c];
    t_labels[tid] = lab, t_ids[tid] = id, t_hits[tid] = hits, t_misses[tid] = misses;
  }
  // every row is written once: a candidate's by the thread of its rank, any other by the thread of the row
  if (tid < ncand) track_id[q_row[tid]] = q_id[tid], track_hits[q_row[tid]] = q_hits[tid];
  if (tid < N && !cand) track_id[tid] = 0, track_hits[tid] = 0;
  if (tid == 0) {
    const int born = min(nb, nf);
    next_id[0] = first_id + born;
    dropped[0] += nb - born;
  }
}
}  // namespace
