// sqlm_bow.cpp — host side of the DBoW2 vocabulary (include/sqrtlm_orb.h:
// sqlm_voc_*, sqlm_bow_transform, sqlm_bow_score): argument checks before the
// device is touched, the breadth-first device layout of the tree, one staged
// upload / launch / read-back per call on the context's stream (kernels:
// sqlm_bow.hip) and the BowVector of each image, which is assembled here from
// the per-feature words in the reference's own order of additions.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

#include "../../include/sqrtlm_orb.h"
#include "sqlm_ctx.h"
#include "sqlm_staging.h"

// Immutable after sqlm_voc_create; owned by a device, shared by its contexts.
struct sqlm_voc {
  int device = 0, k = 0, L = 0;
  int32_t n_nodes = 0, n_words = 0, max_children = 0, max_depth = 0, min_depth = 0;
  char *dev = nullptr;  // descriptors, the node table, the words' weights
  sqlm::BowVocDev d;
};

namespace sqlm {

// the staging buffers of a context's transform and score calls
struct BowSolver {
  Staged in, out;
};

void bow_destroy(BowSolver *s) { delete s; }

namespace {

// The tree as the device reads it. Returns SQLM_OK or the argument error.
struct VocLayout {
  std::vector<BowNode> tab;     // breadth-first
  std::vector<int32_t> order;   // breadth-first position -> caller id
  std::vector<double> word_weight;
  int32_t n_words = 0, max_children = 0, max_depth = 0, min_depth = 0;
};

int voc_layout(int k, int L, int scoring, int weighting, int32_t n, const int32_t *parent, const uint8_t *is_word,
               const uint8_t *desc, const double *weight, VocLayout &V) {
  if (!parent || !is_word || !desc || !weight) return SQLM_ERR_INVALID_ARG;
  if (k < 1 || k > 20 || L < 1 || L > 10 || n < 2) return SQLM_ERR_INVALID_ARG;
  if (scoring != 0 || weighting != 0) return SQLM_ERR_UNSUPPORTED;
  // children of every node in ascending id: a counting sort by parent
  std::vector<int32_t> n_child(n, 0), first(n + 1, 0), depth(n, 0);
  for (int32_t i = 1; i < n; ++i) {
    if (parent[i] < 0 || parent[i] >= i) return SQLM_ERR_INVALID_ARG;
    if (++n_child[parent[i]] > k) return SQLM_ERR_INVALID_ARG;
    depth[i] = depth[parent[i]] + 1;
  }
  V.max_depth = 0;
  V.min_depth = std::numeric_limits<int32_t>::max();
  for (int32_t i = 0; i < n; ++i) {
    const bool w = is_word[i] != 0;
    if (w == (n_child[i] > 0)) return SQLM_ERR_INVALID_ARG;  // a word with children, or a childless node that is no word
    first[i + 1] = first[i] + n_child[i];
    V.max_children = std::max(V.max_children, n_child[i]);
    if (w) {
      V.max_depth = std::max(V.max_depth, depth[i]);
      V.min_depth = std::min(V.min_depth, depth[i]);
    }
  }
  std::vector<int32_t> kids(n - 1), fill(first.begin(), first.end() - 1), word_id(n, -1);
  for (int32_t i = 1; i < n; ++i) kids[fill[parent[i]]++] = i;
  for (int32_t i = 0; i < n; ++i)
    if (is_word[i]) {
      word_id[i] = V.n_words++;
      V.word_weight.push_back(weight[i]);
    }
  // breadth first: every node's children land in one run, in ascending id
  V.order.assign(1, 0);
  V.order.reserve(n);
  V.tab.resize(n);
  for (int32_t pos = 0; pos < n; ++pos) {
    const int32_t id = V.order[pos];
    BowNode &t = V.tab[pos];
    t.child_begin = (int32_t)V.order.size();
    t.child_count = n_child[id];
    t.orig = id;
    t.word = (is_word[id] && weight[id] > 0.0) ? word_id[id] : -1;
    for (int32_t c = first[id]; c < first[id + 1]; ++c) V.order.push_back(kids[c]);
  }
  return SQLM_OK;
}

int bow_solver(sqlm_ctx *c) {
  if (hipSetDevice(c->device) != hipSuccess) return SQLM_ERR_HIP;
  if (!c->bow && !(c->bow = new (std::nothrow) BowSolver)) return SQLM_ERR_OOM;
  return SQLM_OK;
}

// offsets of a CSR array: from 0, ascending
bool csr_ok(const int64_t *off, int n) {
  if (!off || off[0] != 0) return false;
  for (int j = 0; j < n; ++j)
    if (off[j + 1] < off[j]) return false;
  return true;
}

bool words_ok(const int32_t *w, int64_t b, int64_t e) {
  for (int64_t i = b; i < e; ++i)
    if (w[i] < 0 || (i > b && w[i] <= w[i - 1])) return false;
  return true;
}

}  // namespace

}  // namespace sqlm

using namespace sqlm;

extern "C" {

int sqlm_voc_create(int device, int k, int L, int scoring, int weighting, int32_t n_nodes, const int32_t *parent,
                    const uint8_t *is_word, const uint8_t *desc, const double *weight, sqlm_voc **out) {
  if (!out) return SQLM_ERR_INVALID_ARG;
  *out = nullptr;
  VocLayout V;
  if (int r = voc_layout(k, L, scoring, weighting, n_nodes, parent, is_word, desc, weight, V)) return r;
  // the arguments are sound: now the device
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return SQLM_ERR_NO_DEVICE;
  int dev = device;
  if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return SQLM_ERR_HIP;
  if (dev >= n_dev) return SQLM_ERR_INVALID_ARG;
  if (hipSetDevice(dev) != hipSuccess) return SQLM_ERR_HIP;
  sqlm_voc *v = new (std::nothrow) sqlm_voc;
  if (!v) return SQLM_ERR_OOM;
  v->device = dev;
  v->k = k;
  v->L = L;
  v->n_nodes = n_nodes;
  v->n_words = V.n_words;
  v->max_children = V.max_children;
  v->max_depth = V.max_depth;
  v->min_depth = V.min_depth;
  const size_t n = (size_t)n_nodes, desc_bytes = 32 * n, tab_bytes = n * sizeof(BowNode),
               w_bytes = V.word_weight.size() * sizeof(double);
  std::vector<uint8_t> bfs_desc(desc_bytes);
  for (size_t pos = 0; pos < n; ++pos) std::memcpy(&bfs_desc[32 * pos], desc + 32 * (size_t)V.order[pos], 32);
  if (hipMalloc((void **)&v->dev, desc_bytes + tab_bytes + w_bytes) != hipSuccess) {
    delete v;
    return SQLM_ERR_OOM;
  }
  if (hipMemcpy(v->dev, bfs_desc.data(), desc_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(v->dev + desc_bytes, V.tab.data(), tab_bytes, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(v->dev + desc_bytes + tab_bytes, V.word_weight.data(), w_bytes, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(v->dev);
    delete v;
    return SQLM_ERR_HIP;
  }
  v->d.desc = reinterpret_cast<const uint4 *>(v->dev);
  v->d.tab = reinterpret_cast<const BowNode *>(v->dev + desc_bytes);
  v->d.weight = reinterpret_cast<const double *>(v->dev + desc_bytes + tab_bytes);
  v->d.root_count = V.tab[0].child_count;
  v->d.max_depth = V.max_depth;
  *out = v;
  return SQLM_OK;
}

int sqlm_voc_destroy(sqlm_voc *voc) {
  if (!voc) return SQLM_ERR_INVALID_ARG;
  (void)hipSetDevice(voc->device);
  (void)hipDeviceSynchronize();  // a context of this device may still be reading it
  if (voc->dev) (void)hipFree(voc->dev);
  delete voc;
  return SQLM_OK;
}

int sqlm_voc_info(const sqlm_voc *voc, int32_t out[8]) {
  if (!voc || !out) return SQLM_ERR_INVALID_ARG;
  out[0] = voc->k;
  out[1] = voc->L;
  out[2] = voc->n_nodes;
  out[3] = voc->n_words;
  out[4] = voc->max_children;
  out[5] = voc->max_depth;
  out[6] = voc->min_depth;
  out[7] = voc->device;
  return SQLM_OK;
}

int sqlm_bow_transform(sqlm_ctx *c, const sqlm_voc *voc, int n_img, const int64_t *feat_off, const uint8_t *desc,
                       int levelsup, int32_t *word, int32_t *node, int64_t *bow_off, int32_t *bow_word,
                       double *bow_value) {
  if (!c || !voc || n_img < 0 || !bow_off || !csr_ok(feat_off, n_img)) return SQLM_ERR_INVALID_ARG;
  const int64_t n_feat = feat_off[n_img];
  if (n_feat > std::numeric_limits<int32_t>::max()) return SQLM_ERR_INVALID_ARG;
  if (n_feat > 0 && (!desc || !word || !node || !bow_word || !bow_value)) return SQLM_ERR_INVALID_ARG;
  if (c->device != voc->device) return SQLM_ERR_INVALID_ARG;
  for (int j = 0; j <= n_img; ++j) bow_off[j] = 0;
  if (n_feat == 0) return SQLM_OK;  // nothing to descend: the device is not touched

  if (int r = bow_solver(c)) return r;
  BowSolver *s = c->bow;
  const size_t nf = (size_t)n_feat;
  Arena in, out;
  const size_t i_desc = in.take(32 * nf);
  const size_t o_word = out.take(nf * sizeof(int32_t)), o_node = out.take(nf * sizeof(int32_t)),
               o_wt = out.take(nf * sizeof(double));
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->out.grow(out.off)) return r;
  std::memcpy(s->in.host + i_desc, desc, 32 * nf);
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, c->stream));
  // the level whose node the FeatureVector keeps (TemplatedVocabulary.h:1256); the
  // clamp keeps L - levelsup from wrapping and changes no result
  const int nid_level = voc->L - std::max(-(1 << 20), std::min(levelsup, 1 << 20));
  launch_bow_descend(voc->d, at<const uint4>(s->in.dev, i_desc), (int)n_feat, nid_level, at<int32_t>(s->out.dev, o_word),
                     at<int32_t>(s->out.dev, o_node), at<double>(s->out.dev, o_wt), c->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  std::memcpy(word, s->out.host + o_word, nf * sizeof(int32_t));
  std::memcpy(node, s->out.host + o_node, nf * sizeof(int32_t));

  // The BowVector of every image: BowVector::addWeight per feature in feature
  // order (a word seen n times: its weight added n times, not n * w), then
  // BowVector::normalize(L1).
  // The features of an image are ordered by word with a stable radix sort
  // (11-bit digits: two passes for ORBvoc's 10^6 words), so a word's features
  // stay in feature order; a comparison sort of fresh words costs more in
  // mispredicted branches than the descent does on the device.
  constexpr int kDigit = 11;
  int word_bits = 1;
  while (word_bits < 31 && (int64_t(1) << word_bits) < voc->n_words) ++word_bits;
  std::vector<int32_t> idx, tmp;
  uint32_t hist[1 << kDigit];
  const double *wt = at<const double>(s->out.host, o_wt);
  int64_t n_out = 0;
  for (int j = 0; j < n_img; ++j) {
    const int32_t *wj = word + feat_off[j];
    idx.clear();
    for (int64_t i = 0, n = feat_off[j + 1] - feat_off[j]; i < n; ++i)
      if (wj[i] >= 0) idx.push_back((int32_t)i);
    tmp.resize(idx.size());
    for (int shift = 0; shift < word_bits; shift += kDigit) {
      std::memset(hist, 0, sizeof(hist));
      for (int32_t i : idx) ++hist[(wj[i] >> shift) & ((1 << kDigit) - 1)];
      uint32_t run = 0;
      for (uint32_t &h : hist) {
        const uint32_t n = h;
        h = run;
        run += n;
      }
      for (int32_t i : idx) tmp[hist[(wj[i] >> shift) & ((1 << kDigit) - 1)]++] = i;
      idx.swap(tmp);
    }
    const int64_t first = n_out;
    for (size_t a = 0; a < idx.size(); ++a) {
      const double w = wt[feat_off[j] + idx[a]];
      if (a > 0 && wj[idx[a]] == wj[idx[a - 1]]) {
        bow_value[n_out - 1] += w;
      } else {
        bow_word[n_out] = wj[idx[a]];
        bow_value[n_out++] = w;
      }
    }
    double norm = 0.0;
    for (int64_t a = first; a < n_out; ++a) norm += std::fabs(bow_value[a]);
    if (norm > 0.0)
      for (int64_t a = first; a < n_out; ++a) bow_value[a] /= norm;
    bow_off[j + 1] = n_out;
  }
  return SQLM_OK;
}

int sqlm_bow_score(sqlm_ctx *c, int64_t nq, const int32_t *q_word, const double *q_value, int n_db,
                   const int64_t *db_off, const int32_t *db_word, const double *db_value, double *score,
                   int32_t *n_common) {
  if (!c || nq < 0 || nq > std::numeric_limits<int32_t>::max() || n_db < 0) return SQLM_ERR_INVALID_ARG;
  if (nq > 0 && (!q_word || !q_value)) return SQLM_ERR_INVALID_ARG;
  if (!csr_ok(db_off, n_db)) return SQLM_ERR_INVALID_ARG;
  const int64_t n_ent = db_off[n_db];
  if ((n_ent > 0 && (!db_word || !db_value)) || (n_db > 0 && !score)) return SQLM_ERR_INVALID_ARG;
  if (!words_ok(q_word, 0, nq)) return SQLM_ERR_INVALID_ARG;
  for (int j = 0; j < n_db; ++j)
    if (!words_ok(db_word, db_off[j], db_off[j + 1])) return SQLM_ERR_INVALID_ARG;
  if (n_db == 0) return SQLM_OK;
  if (nq == 0 || n_ent == 0) {  // no common word anywhere: the reference's -0.0, without the device
    for (int j = 0; j < n_db; ++j) {
      score[j] = -0.0;
      if (n_common) n_common[j] = 0;
    }
    return SQLM_OK;
  }

  if (int r = bow_solver(c)) return r;
  BowSolver *s = c->bow;
  const size_t q = (size_t)nq, m = (size_t)n_ent, nd = (size_t)n_db;
  Arena in, out;
  const size_t i_qw = in.take(q * sizeof(int32_t)), i_qv = in.take(q * sizeof(double)),
               i_off = in.take((nd + 1) * sizeof(int64_t)), i_dw = in.take(m * sizeof(int32_t)),
               i_dv = in.take(m * sizeof(double));
  const size_t o_score = out.take(nd * sizeof(double)), o_nc = out.take(nd * sizeof(int32_t));
  if (int r = s->in.grow(in.off)) return r;
  if (int r = s->out.grow(out.off)) return r;
  char *h = s->in.host;
  std::memcpy(h + i_qw, q_word, q * sizeof(int32_t));
  std::memcpy(h + i_qv, q_value, q * sizeof(double));
  std::memcpy(h + i_off, db_off, (nd + 1) * sizeof(int64_t));
  std::memcpy(h + i_dw, db_word, m * sizeof(int32_t));
  std::memcpy(h + i_dv, db_value, m * sizeof(double));
  SQLM_HIP_OK(hipMemcpyAsync(s->in.dev, s->in.host, in.off, hipMemcpyHostToDevice, c->stream));
  char *d = s->in.dev;
  launch_bow_score((int)nq, at<const int32_t>(d, i_qw), at<const double>(d, i_qv), n_db, at<const int64_t>(d, i_off),
                   at<const int32_t>(d, i_dw), at<const double>(d, i_dv), at<double>(s->out.dev, o_score),
                   at<int32_t>(s->out.dev, o_nc), c->stream);
  SQLM_HIP_OK(hipGetLastError());
  SQLM_HIP_OK(hipMemcpyAsync(s->out.host, s->out.dev, out.off, hipMemcpyDeviceToHost, c->stream));
  SQLM_HIP_OK(hipStreamSynchronize(c->stream));
  std::memcpy(score, s->out.host + o_score, nd * sizeof(double));
  if (n_common) std::memcpy(n_common, s->out.host + o_nc, nd * sizeof(int32_t));
  return SQLM_OK;
}

}  // extern "C"
