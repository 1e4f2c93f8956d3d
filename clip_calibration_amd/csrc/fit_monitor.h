// The per-epoch tail of the one-call monitored fits (clipmi_adapter_fit_monitored, clipmi_taskres_fit_monitored; DESIGN.md "Fit monitor"):
// behind an epoch's last step the fit's own kernel writes the validation logits into the monitor's workspace, clipmi_val_score turns them into
// epoch record e and, when a best slot is given, clipmi_best_select keeps the parameters of the strictly best epoch.  Host code only; every
// check is made before the run's first launch, with the messages of the two entry points it stands for, so that no epoch can be refused.
#pragma once
#include "common.h"

namespace clipmi {

struct FitMonitor {
  const float* val_feats; int64_t val_ld; const int64_t* val_labels;
  int n_val, n_bins;
  void* records;                // `epochs` epoch records, record e at e * fit_monitor_record_bytes(n_bins)
  int criterion;                // clipmi_best_select's: 0 accuracy, 1 nll
  void* best_block; float* best_params;   // both null: no selection
  void* workspace; size_t workspace_bytes;
};

inline size_t fit_monitor_record_bytes(int n_bins) { return 16 + 16 * ((size_t)n_bins + 1); }

// logits fp32 [n_val, C] | clipmi_val_score's workspace | clipmi_best_select's decision word, each part 256-byte aligned
inline size_t fit_monitor_logits_bytes(int n_val, int C) { return align256((size_t)n_val * (size_t)C * sizeof(float)); }
inline size_t fit_monitor_bytes(int n_val, int C, int n_bins) {
  const size_t score = clipmi_val_score_workspace_bytes(n_val, n_bins);
  if (C < 1 || score == 0) return 0;
  return fit_monitor_logits_bytes(n_val, C) + score + clipmi_best_select_workspace_bytes(1);
}

inline int check_fit_monitor(const char* who, const FitMonitor& m, int E, int C) {
  CLIPMI_REQUIRE(m.val_feats && m.val_labels && m.records && m.workspace, CLIPMI_ERR_ARG,
                 "%s: null pointer (the validation features and labels, the records and the monitor's workspace are required)", who);
  CLIPMI_REQUIRE((m.best_block == nullptr) == (m.best_params == nullptr), CLIPMI_ERR_ARG,
                 "%s: the best block and the best slot come together (both or neither)", who);
  CLIPMI_REQUIRE((uintptr_t)m.val_feats % 4 == 0, CLIPMI_ERR_ARG, "%s: fp32 arrays must be 4-byte aligned, the labels 8-byte aligned", who);
  CLIPMI_REQUIRE(((uintptr_t)m.val_labels | (uintptr_t)m.records | (uintptr_t)m.best_block) % 8 == 0, CLIPMI_ERR_ARG,
                 "%s: the validation labels, the records and the best block must be 8-byte aligned", who);
  CLIPMI_REQUIRE((uintptr_t)m.best_params % 16 == 0, CLIPMI_ERR_ARG, "%s: params and best_params must be 16-byte aligned", who);
  CLIPMI_REQUIRE((uintptr_t)m.workspace % 256 == 0, CLIPMI_ERR_ARG, "%s: the monitor's workspace must be 256-byte aligned", who);
  CLIPMI_REQUIRE(m.n_bins >= 1 && m.n_bins <= 64, CLIPMI_ERR_ARG, "%s: n_bins=%d outside 1..64", who, m.n_bins);
  CLIPMI_REQUIRE(m.criterion == 0 || m.criterion == 1, CLIPMI_ERR_ARG, "%s: criterion=%d (0: accuracy, 1: nll)", who, m.criterion);
  CLIPMI_REQUIRE(m.n_val >= 1, CLIPMI_ERR_SHAPE, "%s: N_val=%d (>= 1)", who, m.n_val);
  CLIPMI_REQUIRE(m.val_ld >= E, CLIPMI_ERR_SHAPE, "%s: validation ld=%lld < E=%d", who, (long long)m.val_ld, E);
  const size_t need = fit_monitor_bytes(m.n_val, C, m.n_bins);
  CLIPMI_REQUIRE(m.workspace_bytes >= need, CLIPMI_ERR_WORKSPACE, "%s: monitor workspace of %zu bytes, %zu needed", who, m.workspace_bytes, need);
  return CLIPMI_OK;
}

inline float* fit_monitor_logits(const FitMonitor& m) { return static_cast<float*>(m.workspace); }

// behind the validation logits of epoch e: the record and, with a best slot, the selection of params [n_floats]
inline int fit_monitor_score(const FitMonitor& m, int e, int C, const float* params, int64_t n_floats, clipmi_stream_t stream) {
  char* ws = static_cast<char*>(m.workspace) + fit_monitor_logits_bytes(m.n_val, C);
  const size_t score = clipmi_val_score_workspace_bytes(m.n_val, m.n_bins);
  void* record = static_cast<char*>(m.records) + (size_t)e * fit_monitor_record_bytes(m.n_bins);
  if (int rc = clipmi_val_score(fit_monitor_logits(m), C, m.val_labels, m.n_val, C, m.n_bins, record, ws, score, stream)) return rc;
  if (!m.best_block) return CLIPMI_OK;
  return clipmi_best_select(record, m.best_block, m.criterion, e, params, m.best_params, n_floats, ws + score, clipmi_best_select_workspace_bytes(1),
                            stream);
}

}  // namespace clipmi
