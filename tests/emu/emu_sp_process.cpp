// Host build of csrc/sp_process_math.h: a stand-alone program that runs the launches of csrc/sp_process.hip one image at a time
// over records read from a file.  tests/test_sp_process_ref_cpu.py feeds it and checks the output through the same check() as
// the GPU; it is also built with -fsanitize=address,undefined and run on its own.
//   usage: emu_sp_process <in> <out>
//   record 1 (nms): int32 1, H, W, d, r; float thr, heat[H*W]
//     -> int32 rounds, count; uint8 map[H*W]; int32 pts[2*count]; float conf[count]
//     The rounds here are synchronous (every decision of a round reads the states of the round before): the longest schedule
//     the device can take; `rounds` counts them.
//   record 2 (soft-argmax and its adjoint): int32 2, H, W, p, n; float heat[H*W]; int32 pts[2n]; float g_pred[2n]
//     -> float pred[2n], g_heat[H*W]
//   record 3 (descriptor sampling): int32 3, Hc, Wc, D, align_corners, n; float desc[D*Hc*Wc]; double xy[2n] -> float out[n*D]
//   record 4 (flatten and its adjoint): int32 4, Hc, Wc; float semi[65*Hc*Wc], g_heat[64*Hc*Wc] -> float heat[64*Hc*Wc], g_semi[65*Hc*Wc]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sp_process_math.h"

namespace {

struct Reader {
  std::vector<unsigned char> buf;
  size_t off = 0;
  template <class T>
  bool take(T* out, size_t count) {
    if (count == 0) return true;
    if (off + count * sizeof(T) > buf.size()) return false;
    std::memcpy(out, buf.data() + off, count * sizeof(T));
    off += count * sizeof(T);
    return true;
  }
};

template <class T>
void put(std::vector<unsigned char>& out, const T* v, size_t count) {
  if (count == 0) return;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v);
  out.insert(out.end(), p, p + count * sizeof(T));
}

bool nms(Reader& in, std::vector<unsigned char>& out) {
  int hdr[4];
  float thr;
  if (!in.take(hdr, 4) || !in.take(&thr, 1)) return false;
  const int H = hdr[0], W = hdr[1], d = hdr[2], r = hdr[3];
  if (H < 1 || W < 1 || d < 0 || r < 0) return false;
  const size_t n = (size_t)H * W;
  std::vector<float> heat(n);
  if (!in.take(heat.data(), n)) return false;
  std::vector<unsigned char> state(n), next(n);
  for (size_t i = 0; i < n; ++i) state[i] = sp::candidate(heat[i], thr) ? sp::kUndecided : sp::kNone;
  int rounds = 0;
  for (;;) {
    bool pending = false, any = false;
    next = state;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        if (state[i] != sp::kUndecided) continue;
        any = true;
        next[i] = sp::decide_pixel(heat.data(), state.data(), H, W, d, y, x);
        if (next[i] == sp::kUndecided) pending = true;
      }
    state.swap(next);
    if (any) ++rounds;
    if (!pending) break;
  }
  std::vector<unsigned char> map(n, 0);
  std::vector<int> pts;
  std::vector<float> conf;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t i = (size_t)y * W + x;
      if (state[i] == sp::kKept && sp::inside_border(y, x, H, W, r)) {
        map[i] = 1;
        pts.push_back(x);
        pts.push_back(y);
        conf.push_back(heat[i]);
      }
    }
  const int count = (int)conf.size();
  if ((long)count > sp::nms_capacity(H, W, d)) return false;
  put(out, &rounds, 1);
  put(out, &count, 1);
  put(out, map.data(), n);
  put(out, pts.data(), pts.size());
  put(out, conf.data(), conf.size());
  return true;
}

bool soft_argmax(Reader& in, std::vector<unsigned char>& out) {
  int hdr[4];
  if (!in.take(hdr, 4)) return false;
  const int H = hdr[0], W = hdr[1], p = hdr[2], np = hdr[3];
  if (H < 1 || W < 1 || p < 1 || p % 2 == 0 || np < 0) return false;
  const size_t n = (size_t)H * W;
  const int c = p / 2;
  std::vector<float> heat(n), g(2 * (size_t)np);
  std::vector<int> pts(2 * (size_t)np);
  if (!in.take(heat.data(), n) || !in.take(pts.data(), pts.size()) || !in.take(g.data(), g.size())) return false;
  std::vector<int> index(n, -1);
  std::vector<sp::Patch> rec(np);
  std::vector<double> share(np);
  std::vector<float> pred(2 * (size_t)np, 0.0f), gh(n);
  for (int k = 0; k < np; ++k) {
    const int x = pts[2 * k], y = pts[2 * k + 1];
    if (x < c || y < c || x >= W - c || y >= H - c) return false;
    rec[k] = sp::soft_argmax(heat.data(), W, x, y, p);
    share[k] = rec[k].valid ? sp::grad_norm_share(rec[k], heat.data(), W, x, y, p, g[2 * k], g[2 * k + 1]) : 0.0;
    if (rec[k].valid) {
      pred[2 * k] = (float)(rec[k].ox - (double)c);
      pred[2 * k + 1] = (float)(rec[k].oy - (double)c);
    }
    index[(size_t)y * W + x] = k;
  }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      double acc = 0.0;
      for (int cy = y - c < 0 ? 0 : y - c; cy <= (y + c > H - 1 ? H - 1 : y + c); ++cy)
        for (int cx = x - c < 0 ? 0 : x - c; cx <= (x + c > W - 1 ? W - 1 : x + c); ++cx) {
          const int k = index[(size_t)cy * W + cx];
          if (k < 0 || !rec[k].valid) continue;
          acc += sp::grad_h(rec[k], (double)heat[(size_t)y * W + x], x - cx + c, y - cy + c, g[2 * k], g[2 * k + 1], share[k]);
        }
      gh[(size_t)y * W + x] = (float)acc;
    }
  put(out, pred.data(), pred.size());
  put(out, gh.data(), gh.size());
  return true;
}

bool sample(Reader& in, std::vector<unsigned char>& out) {
  int hdr[5];
  if (!in.take(hdr, 5)) return false;
  const int Hc = hdr[0], Wc = hdr[1], D = hdr[2], align = hdr[3], np = hdr[4];
  if (Hc < 1 || Wc < 1 || D < 1 || np < 0) return false;
  const size_t plane = (size_t)Hc * Wc;
  std::vector<float> desc(D * plane), res((size_t)np * D);
  std::vector<double> xy(2 * (size_t)np), v(D);
  if (!in.take(desc.data(), desc.size()) || !in.take(xy.data(), xy.size())) return false;
  for (int k = 0; k < np; ++k) {
    const sp::Taps t = sp::bilinear_taps(xy[2 * k], xy[2 * k + 1], Hc, Wc, align);
    double ss = 0.0;
    for (int ch = 0; ch < D; ++ch) {
      v[ch] = sp::sample(desc.data() + ch * plane, Hc, Wc, t);
      ss += v[ch] * v[ch];
    }
    const double norm = sqrt(ss);
    for (int ch = 0; ch < D; ++ch) res[(size_t)k * D + ch] = norm > 0.0 ? (float)(v[ch] / norm) : 0.0f;
  }
  put(out, res.data(), res.size());
  return true;
}

bool flatten(Reader& in, std::vector<unsigned char>& out) {
  int hdr[2];
  if (!in.take(hdr, 2)) return false;
  const int Hc = hdr[0], Wc = hdr[1];
  if (Hc < 1 || Wc < 1) return false;
  const long cells = (long)Hc * Wc, W = 8L * Wc;
  std::vector<float> semi(65 * cells), g(64 * cells), heat(64 * cells), gs(65 * cells);
  if (!in.take(semi.data(), semi.size()) || !in.take(g.data(), g.size())) return false;
  for (int hc = 0; hc < Hc; ++hc)
    for (int wc = 0; wc < Wc; ++wc) {
      const float* v = semi.data() + (long)hc * Wc + wc;
      const double m = sp::cell_max(v, cells), s = sp::cell_sum(v, cells, m);
      const long at = (long)hc * 8 * W + (long)wc * 8;
      const double dot = sp::cell_dot(v, cells, m, s, g.data() + at, W);
      for (int c = 0; c < 65; ++c) {
        const float vc = v[c * cells];
        const double pc = sp::cell_prob(vc, m, s);
        const double gc = c < 64 ? (double)g[at + (c / 8) * W + (c % 8)] : 0.0;
        if (c < 64) heat[at + (c / 8) * W + (c % 8)] = (float)pc;
        gs[(long)c * cells + (long)hc * Wc + wc] = (vc != vc) ? 0.0f : (float)(pc * (gc - dot));
      }
    }
  put(out, heat.data(), heat.size());
  put(out, gs.data(), gs.size());
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]);
    return 2;
  }
  Reader in;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  unsigned char chunk[1 << 16];
  size_t got;
  while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) in.buf.insert(in.buf.end(), chunk, chunk + got);
  std::fclose(f);
  std::vector<unsigned char> out;
  while (in.off < in.buf.size()) {
    int kind = 0;
    if (!in.take(&kind, 1)) return 3;
    bool ok = false;
    if (kind == 1) ok = nms(in, out);
    else if (kind == 2) ok = soft_argmax(in, out);
    else if (kind == 3) ok = sample(in, out);
    else if (kind == 4) ok = flatten(in, out);
    if (!ok) {
      std::fprintf(stderr, "bad record of kind %d at byte %zu\n", kind, in.off);
      return 3;
    }
  }
  f = std::fopen(argv[2], "wb");
  if (!f) return 2;
  if (!out.empty() && std::fwrite(out.data(), 1, out.size(), f) != out.size()) return 2;
  std::fclose(f);
  return 0;
}
