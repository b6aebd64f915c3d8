// sdc_mirror.hpp -- WHAT THE HOST KNOWS OF EACH ENV.  The library never reads the device back to decide what to do next: when an episode
// ends and the auto-reset launches, whether the batch is in lock-step (rel_hint -> sdc_dispatch.hpp -> which kernel), what a snapshot's
// manifest records, whether a mark is alive, whether a replica group is in step -- all of it is decided from this copy.  An error in it
// raises no error anywhere, so the copy is ONE type whose operations are the ones the entry points perform, each keeping the invariants
// below by itself: no caller folds, recomputes or counts by hand.
//
// Plain C++17: no HIP, no sdc_handle, no device calls, no messages -- a host compiler alone builds it (tests/test_host_mirror.py holds
// it to a model restated in Python without a GPU; tests/test_gpu_host_mirror.py holds the library's copy to the device's arrays).
// DESIGN.md section 4.17 lists which entry point uses which operation.
//
// Invariants
//   * env e is at episode step base_[e] + pending_ (t_rel).  Every env advances one step per launched step, so a stepping call adds to
//     pending_ alone: O(1).  The FOLD (pending_ into base_) happens when an episode ends and before any operation writes a single env's
//     step; a read never needs it.
//   * steps_to_terminal = episode_steps - max t_rel and rel_hint = the common t_rel (-1: not in lock-step) are DERIVED.  Stepping
//     updates them incrementally (exact: every env advances alike); every operation that writes an env's step recomputes them.  They
//     mean something from the first reset (or reload) on: a fresh mirror has every env "finished" (t_rel = episode_steps), 0 steps left
//     and no rel_hint.
//   * n_feat counts the envs whose episode has valid feature rows (feat_).  An engine without feature rows never notes any.
//   * config and location ids are unassigned (read as 0) until the first assignment; an env replacement does not assign them.
//   * ONE live mark per env: mark_serial_[e] is the serial of the env's latest mark, 0 for none (sized by the first mark).  A mark dies
//     by a later mark of the env, a new episode (reset, auto-reset), a replacement of the env, kill / kill_all; a rewind keeps it.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

// what an env holds after it has been replaced as a whole (sdc_restore_envs: from the row's manifest)
struct SdcEnvFacts {
  int env, t_rel;
  bool feat_ok;
  int cfg, loc;
};

class SdcHostMirror {
 public:
  SdcHostMirror() = default;
  // N envs, all "finished": a reset is required before stepping.  has_feat: the engine keeps feature rows at all
  SdcHostMirror(const int n_envs, const int episode_steps, const bool has_feat)
      : n_(n_envs), episode_steps_(episode_steps), has_feat_(has_feat), base_((size_t)n_envs, episode_steps), feat_((size_t)n_envs, 0),
        last_done_((size_t)n_envs, 0) {}

  // ---- reads ---------------------------------------------------------------------------------------------------------------------------
  int t_rel(const int e) const { return base_[(size_t)e] + pending_; }
  bool feat(const int e) const { return feat_[(size_t)e] != 0; }
  int cfg(const int e) const { return cfg_.empty() ? 0 : cfg_[(size_t)e]; }
  int loc(const int e) const { return loc_.empty() ? 0 : loc_[(size_t)e]; }
  const int* cfg_ids() const { return cfg_.empty() ? nullptr : cfg_.data(); }      // [N], or nullptr: unassigned
  int rel_hint() const { return rel_hint_; }
  int steps_to_terminal() const { return steps_to_terminal_; }
  int n_feat() const { return n_feat_; }
  // the envs that finished in the last stepping call: how many, and (meaningful while that is > 0) which
  int n_last_done() const { return n_last_done_; }
  const unsigned char* last_done() const { return last_done_.data(); }

  // ---- assignment (ids[e * stride]: a dense array, or a field of the envs' records) ---------------------------------------------------
  void set_cfg_ids(const int* ids, const size_t stride = 1) { gather(cfg_, ids, stride); }
  void set_loc_ids(const int* ids, const size_t stride = 1) { gather(loc_, ids, stride); }

  // ---- stepping ------------------------------------------------------------------------------------------------------------------------
  // n steps were launched (1 <= n <= steps_to_terminal).  -> an env just finished; then last_done / n_last_done name the finished envs
  bool stepped(const int n) {
    n_last_done_ = 0;
    steps_to_terminal_ -= n;
    pending_ += n;
    if (rel_hint_ >= 0) rel_hint_ += n;
    if (steps_to_terminal_ != 0) return false;
    fold();
    for (int e = 0; e < n_; e++) {
      last_done_[(size_t)e] = base_[(size_t)e] >= episode_steps_;
      n_last_done_ += last_done_[(size_t)e];
    }
    return true;
  }
  // the envs that have finished their episode have been reset (auto_reset, behind a stepped() that returned true)
  void finished_envs_reset() {
    fold();
    for (int e = 0; e < n_; e++)
      if (base_[(size_t)e] >= episode_steps_) new_episode(e);
    recompute();
  }

  // ---- reset: new episodes for the masked envs (mask == nullptr: the whole batch) -----------------------------------------------------
  void reset(const unsigned char* mask) {
    fold();
    for (int e = 0; e < n_; e++)
      if (!mask || mask[e]) new_episode(e);
    recompute();
  }

  // ---- whole envs replaced: their marks die, lock-step comes back if the batch is in it afterwards ------------------------------------
  // env dst[k] has become a copy of env src[k] (no env is both)
  void copy_envs(const int* src, const int* dst, const int n) {
    fold();
    for (int k = 0; k < n; k++) follow({dst[k], base_[(size_t)src[k]], feat(src[k]), cfg(src[k]), loc(src[k])});
    recompute();
  }
  // env f[k].env holds what f[k] says
  void replace_envs(const SdcEnvFacts* f, const size_t n) {
    fold();
    for (size_t k = 0; k < n; k++) follow(f[k]);
    recompute();
  }

  // ---- rewind: env envs[k] (nullptr: env k) is back at episode step t_rel[k * stride]; its mark stays alive --------------------------
  void rewind(const int* envs, const int n, const int* t_rel, const size_t stride = 1) {
    fold();
    for (int k = 0; k < n; k++) base_[(size_t)(envs ? envs[k] : k)] = t_rel[(size_t)k * stride];
    recompute();
  }

  // ---- every env's episode step reloaded (the steps launched since the last fold are dropped with the old values) --------------------
  void reload_t_rel(const int* t_rel) {
    pending_ = 0;
    base_.assign(t_rel, t_rel + n_);
    recompute();
  }

  // ---- no env has valid feature rows any more ------------------------------------------------------------------------------------------
  void features_invalidated() {
    std::fill(feat_.begin(), feat_.end(), 0);
    n_feat_ = 0;
  }

  // ---- marks ---------------------------------------------------------------------------------------------------------------------------
  static constexpr int next_serial(const int s) { return s == 0x7FFFFFFF ? 1 : s + 1; }      // (never 0)
  // a mark of envs[0 .. n) (nullptr: of the whole batch) -> its serial; the envs' earlier marks are dead
  int mark(const int* envs, const int n) {
    if (mark_serial_.empty()) mark_serial_.assign((size_t)n_, 0);
    mark_next_serial_ = next_serial(mark_next_serial_);
    for (int k = 0; k < (envs ? n : n_); k++) mark_serial_[(size_t)(envs ? envs[k] : k)] = mark_next_serial_;
    return mark_next_serial_;
  }
  bool mark_alive(const int e, const int serial) const {
    return serial != 0 && !mark_serial_.empty() && mark_serial_[(size_t)e] == serial;
  }
  // the steps env e has taken since it was at episode step t_rel_then of this episode (negative: it is before that step)
  int steps_since(const int e, const int t_rel_then) const { return t_rel(e) - t_rel_then; }
  void mark_kill(const int e) {
    if (!mark_serial_.empty()) mark_serial_[(size_t)e] = 0;
  }
  void mark_kill_all() { std::fill(mark_serial_.begin(), mark_serial_.end(), 0); }

 private:
  void fold() {
    if (pending_) {
      for (int& t : base_) t += pending_;
      pending_ = 0;
    }
  }
  void recompute() {      // (folded)
    if (base_.empty()) return;      // (a default-constructed mirror: no envs, nothing derived)
    int most = base_[0];
    bool lock_step = true;
    for (const int t : base_) {
      most = std::max(most, t);
      lock_step = lock_step && t == base_[0];
    }
    steps_to_terminal_ = episode_steps_ - most;
    rel_hint_ = lock_step ? base_[0] : -1;
  }
  void set_feat(const int e, const bool ok) {
    n_feat_ += (int)ok - (int)feat(e);
    feat_[(size_t)e] = ok;
  }
  // env e has started a new episode: whatever a reset invalidates
  void new_episode(const int e) {
    base_[(size_t)e] = 0;
    if (has_feat_) set_feat(e, true);      // (the reset kernels are followed by the features kernel)
    mark_kill(e);
  }
  // env f.env's state has been replaced as a whole
  void follow(const SdcEnvFacts& f) {
    base_[(size_t)f.env] = f.t_rel;
    mark_kill(f.env);
    set_feat(f.env, has_feat_ && f.feat_ok);
    if (!cfg_.empty()) cfg_[(size_t)f.env] = f.cfg;
    if (!loc_.empty()) loc_[(size_t)f.env] = f.loc;
  }
  void gather(std::vector<int>& to, const int* ids, const size_t stride) const {
    to.resize((size_t)n_);
    for (int e = 0; e < n_; e++) to[(size_t)e] = ids[(size_t)e * stride];
  }

  int n_ = 0, episode_steps_ = 0;
  bool has_feat_ = false;
  std::vector<int> base_;      // [N] episode step at the last fold
  int pending_ = 0;            // steps launched since
  int steps_to_terminal_ = 0, rel_hint_ = -1;
  std::vector<unsigned char> feat_;
  int n_feat_ = 0;
  std::vector<int> cfg_, loc_;      // [N], or empty: unassigned
  std::vector<unsigned char> last_done_;
  int n_last_done_ = 0;
  std::vector<int> mark_serial_;      // [N], or empty: no mark yet
  int mark_next_serial_ = 0;
};
