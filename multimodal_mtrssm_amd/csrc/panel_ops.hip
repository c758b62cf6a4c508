// Episode panels for gfx950: the finished uint8 video `prior | observation | posterior (| error)`, vision on the
// top row and magma-coloured audio on the bottom row, from the decoders' activated fp32 frames in ONE launch -- denormalise, quantise,
// colormap lookup, nearest-neighbour upscale, tiling, separators, phase bar and frame number.  Replaces the reference callback's host
// composition (mrssm/callback.py:250-340 create_multimodal_combined_video, 689-905 log_multimodal_video and the numpy / matplotlib /
// PIL loops below it).
//
// Launch shape: the video is one flat array of P = N T Hc Wc pixels.  A lane owns 4 consecutive pixels = 12 bytes = 3 whole dwords at a
// 4-byte aligned offset (12 * unit), so a wave stores 768 contiguous bytes and no row or frame needs padding in memory: a lane's pixels
// may straddle a row or a frame, the position is carried like an odometer.  Only the video's last 1 .. 3 pixels (P no multiple of 4)
// leave fewer than 4 bytes at the very end; those -- at most 3 bytes of the whole launch -- are byte stores, everything else is a dword.
// A source element that serves `scale` neighbouring pixels of a row is read and coloured once per lane and reused.  The magma table sits
// in LDS (a divergent index costs nothing there).  No atomics: every byte is a function of the inputs alone.
//
// The pixel rule is fp32 in a fixed order with correctly rounded division, no FMA contraction (the whole file is compiled with
// contraction off): it must give the reference's bytes exactly.
#include "scan_common.h"

#pragma clang fp contract(off)

namespace mtrssm {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;   // grid-stride above this
constexpr int kMaxCanvas = 32768;  // Hc, Wc at most (the reciprocal divisions below are exact far beyond it)
constexpr int kMaxScale = 64, kMaxGap = 64, kMaxBar = 64, kMaxLabel = 16;

// trunc(matplotlib magma(k)[:3] * 255), k = 0 .. 255
__constant__ unsigned char kMagma[256][3] = {
    {0, 0, 3}, {0, 0, 4}, {0, 0, 6}, {1, 0, 7}, {1, 1, 9}, {1, 1, 11}, {2, 2, 13}, {2, 2, 15},
    {3, 3, 17}, {4, 3, 19}, {4, 4, 21}, {5, 4, 23}, {6, 5, 25}, {7, 5, 27}, {8, 6, 29}, {9, 7, 31},
    {10, 7, 34}, {11, 8, 36}, {12, 9, 38}, {13, 10, 40}, {14, 10, 42}, {15, 11, 44}, {16, 12, 47}, {17, 12, 49},
    {18, 13, 51}, {20, 13, 53}, {21, 14, 56}, {22, 14, 58}, {23, 15, 60}, {24, 15, 63}, {26, 16, 65}, {27, 16, 68},
    {28, 16, 70}, {30, 16, 73}, {31, 17, 75}, {32, 17, 77}, {34, 17, 80}, {35, 17, 82}, {37, 17, 85}, {38, 17, 87},
    {40, 17, 89}, {42, 17, 92}, {43, 17, 94}, {45, 16, 96}, {47, 16, 98}, {48, 16, 101}, {50, 16, 103}, {52, 16, 104},
    {53, 15, 106}, {55, 15, 108}, {57, 15, 110}, {59, 15, 111}, {60, 15, 113}, {62, 15, 114}, {64, 15, 115}, {66, 15, 116},
    {67, 15, 117}, {69, 15, 118}, {71, 15, 119}, {72, 16, 120}, {74, 16, 121}, {75, 16, 121}, {77, 17, 122}, {79, 17, 123},
    {80, 18, 123}, {82, 18, 124}, {83, 19, 124}, {85, 19, 125}, {87, 20, 125}, {88, 21, 126}, {90, 21, 126}, {91, 22, 126},
    {93, 23, 126}, {94, 23, 127}, {96, 24, 127}, {97, 24, 127}, {99, 25, 127}, {101, 26, 128}, {102, 26, 128}, {104, 27, 128},
    {105, 28, 128}, {107, 28, 128}, {108, 29, 128}, {110, 30, 129}, {111, 30, 129}, {113, 31, 129}, {115, 31, 129}, {116, 32, 129},
    {118, 33, 129}, {119, 33, 129}, {121, 34, 129}, {122, 34, 129}, {124, 35, 129}, {126, 36, 129}, {127, 36, 129}, {129, 37, 129},
    {130, 37, 129}, {132, 38, 129}, {133, 38, 129}, {135, 39, 129}, {137, 40, 129}, {138, 40, 129}, {140, 41, 128}, {141, 41, 128},
    {143, 42, 128}, {145, 42, 128}, {146, 43, 128}, {148, 43, 128}, {149, 44, 128}, {151, 44, 127}, {153, 45, 127}, {154, 45, 127},
    {156, 46, 127}, {158, 46, 126}, {159, 47, 126}, {161, 47, 126}, {163, 48, 126}, {164, 48, 125}, {166, 49, 125}, {167, 49, 125},
    {169, 50, 124}, {171, 51, 124}, {172, 51, 123}, {174, 52, 123}, {176, 52, 123}, {177, 53, 122}, {179, 53, 122}, {181, 54, 121},
    {182, 54, 121}, {184, 55, 120}, {185, 55, 120}, {187, 56, 119}, {189, 57, 119}, {190, 57, 118}, {192, 58, 117}, {194, 58, 117},
    {195, 59, 116}, {197, 60, 116}, {198, 60, 115}, {200, 61, 114}, {202, 62, 114}, {203, 62, 113}, {205, 63, 112}, {206, 64, 112},
    {208, 65, 111}, {209, 66, 110}, {211, 66, 109}, {212, 67, 109}, {214, 68, 108}, {215, 69, 107}, {217, 70, 106}, {218, 71, 105},
    {220, 72, 105}, {221, 73, 104}, {222, 74, 103}, {224, 75, 102}, {225, 76, 102}, {226, 77, 101}, {228, 78, 100}, {229, 80, 99},
    {230, 81, 98}, {231, 82, 98}, {232, 84, 97}, {234, 85, 96}, {235, 86, 96}, {236, 88, 95}, {237, 89, 95}, {238, 91, 94},
    {238, 93, 93}, {239, 94, 93}, {240, 96, 93}, {241, 97, 92}, {242, 99, 92}, {243, 101, 92}, {243, 103, 91}, {244, 104, 91},
    {245, 106, 91}, {245, 108, 91}, {246, 110, 91}, {246, 112, 91}, {247, 113, 91}, {247, 115, 92}, {248, 117, 92}, {248, 119, 92},
    {249, 121, 92}, {249, 123, 93}, {249, 125, 93}, {250, 127, 94}, {250, 128, 94}, {250, 130, 95}, {251, 132, 96}, {251, 134, 96},
    {251, 136, 97}, {251, 138, 98}, {252, 140, 99}, {252, 142, 99}, {252, 144, 100}, {252, 146, 101}, {252, 147, 102}, {253, 149, 103},
    {253, 151, 104}, {253, 153, 105}, {253, 155, 106}, {253, 157, 107}, {253, 159, 108}, {253, 161, 110}, {253, 162, 111}, {253, 164, 112},
    {254, 166, 113}, {254, 168, 115}, {254, 170, 116}, {254, 172, 117}, {254, 174, 118}, {254, 175, 120}, {254, 177, 121}, {254, 179, 123},
    {254, 181, 124}, {254, 183, 125}, {254, 185, 127}, {254, 187, 128}, {254, 188, 130}, {254, 190, 131}, {254, 192, 133}, {254, 194, 134},
    {254, 196, 136}, {254, 198, 137}, {254, 199, 139}, {254, 201, 141}, {254, 203, 142}, {253, 205, 144}, {253, 207, 146}, {253, 209, 147},
    {253, 210, 149}, {253, 212, 151}, {253, 214, 152}, {253, 216, 154}, {253, 218, 156}, {253, 220, 157}, {253, 221, 159}, {253, 223, 161},
    {253, 225, 163}, {252, 227, 165}, {252, 229, 166}, {252, 230, 168}, {252, 232, 170}, {252, 234, 172}, {252, 236, 174}, {252, 238, 176},
    {252, 240, 177}, {252, 241, 179}, {252, 243, 181}, {252, 245, 183}, {251, 247, 185}, {251, 249, 187}, {251, 250, 189}, {251, 252, 191}};

// The 3 x 5 font of the frame number: digit d, row r (top to bottom), column c (left to right) is bit 14 - (3 r + c).
__constant__ unsigned short kFont[10] = {
    0x7B6F,  // 0: 111 101 101 101 111
    0x2C97,  // 1: 010 110 010 010 111
    0x73E7,  // 2: 111 001 111 100 111
    0x73CF,  // 3: 111 001 111 001 111
    0x5BC9,  // 4: 101 101 111 001 001
    0x79CF,  // 5: 111 100 111 001 111
    0x79EF,  // 6: 111 100 111 101 111
    0x7249,  // 7: 111 001 001 001 001
    0x7BEF,  // 8: 111 101 111 101 111
    0x7BCF,  // 9: 111 101 111 001 111
};

constexpr uint32_t kGapColour = 64u | (64u << 8) | (64u << 16);
constexpr uint32_t kBarContext = 0u | (160u << 8) | (0u << 16);
constexpr uint32_t kBarOpen = 255u | (140u << 8) | (0u << 16);
constexpr uint32_t kWhite = 0xFFFFFFu;

struct PanelArgs {
  const float* src[2][3];  // [audio, vision][prior, observation, posterior]
  const int32_t* codes;
  const int32_t* valid;
  const int32_t* context;
  unsigned char* out;
  int64_t pixels;          // N T Hc Wc
  int64_t frame_elems[2];  // C H W
  int32_t plane[2];        // H W
  int32_t C[2], H[2], W[2];
  int32_t T, Hc, Wc, cw, hv, scale, gap, bar, label, frame0, n_columns, blank_unseen;
  int32_t columns[4];
  uint32_t inv_scale, inv_label;  // ceil(2^32 / d) (unused when d = 1)
};

// x / d for x < 2^16, 2 <= d <= 64 by the reciprocal m = ceil(2^32 / d): m d - 2^32 < d, so the quotient is exact while x d < 2^32.
__device__ __forceinline__ int div_small(int x, uint32_t inv, int d) { return d == 1 ? x : (int)__umulhi((uint32_t)x, inv); }

// v in [-1, 1] -> [0, 1]; NaN -> 0
__device__ __forceinline__ float to_unit(float v) {
  float x = (v + 1.0f) / 2.0f;
  x = x > 0.0f ? x : 0.0f;
  return x < 1.0f ? x : 1.0f;
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) {
  x = x > lo ? x : lo;
  return x < hi ? x : hi;
}

__device__ __forceinline__ uint32_t magma_of(float s, const uint32_t* lut) {
  int i = (int)(s * 256.0f);
  return lut[i < 255 ? i : 255];
}

__device__ __forceinline__ uint32_t audio_colour(float x, const uint32_t* lut) {
  const float n = x * 2.0f - 1.0f;
  const float db = (n + 1.0f) / 2.0f * 80.0f - 80.0f;
  const float s = clampf((clampf(db, -80.0f, 0.0f) - (-80.0f)) / 80.0f, 0.0f, 1.0f);
  return magma_of(s, lut);
}

// What a frame decides for all its pixels.
struct FrameState {
  int64_t base[2];  // element offset of the frame in the audio / vision inputs
  int value;        // the number drawn: frame0 + t
  int digits;       // its decimal digits
  int box_w;        // the label's box, in pixels (0: none)
  uint32_t bar;     // the bar's colour
  int code;         // seen bits
  bool dead;
};

__device__ __forceinline__ FrameState frame_state(const PanelArgs& a, int f) {
  FrameState s;
  const int n = f / a.T, t = f - n * a.T;
  s.base[0] = (int64_t)f * a.frame_elems[0];
  s.base[1] = (int64_t)f * a.frame_elems[1];
  int len = a.T;
  if (a.valid) {
    len = a.valid[n];
    len = len < 0 ? 0 : len;
  }
  s.dead = t >= len;
  s.bar = t < a.context[n] ? kBarContext : kBarOpen;
  s.code = a.codes ? a.codes[f] : 3;
  s.value = a.frame0 + t;
  int digits = 1;
  for (int v = s.value; v >= 10; v /= 10) ++digits;
  s.digits = digits;
  s.box_w = a.label * (4 * digits + 1);
  return s;
}

// What a canvas row decides: which band it lies in and the source row.
struct RowState {
  int band;  // 0 audio cells, 1 vision cells, 2 bar, 3 gap
  int sy;
};

__device__ __forceinline__ RowState row_state(const PanelArgs& a, int y) {
  RowState r;
  r.sy = 0;
  if (y < a.bar) { r.band = 2; return r; }
  y -= a.bar;
  if (y < a.hv) { r.band = 1; r.sy = div_small(y, a.inv_scale, a.scale); return r; }
  y -= a.hv;
  if (y < a.gap) { r.band = 3; return r; }
  r.band = 0;
  r.sy = div_small(y - a.gap, a.inv_scale, a.scale);
  return r;
}

// The frames of modality m in kind k (prior, observation, posterior), picked by selects: an index that differs from lane to lane
// into the kernel's arguments would send them through scratch memory.
__device__ __forceinline__ const float* frames_of(const PanelArgs& a, int m, int k) {
  const float* pa = k == MTRSSM_PANEL_PRIOR ? a.src[0][0] : k == MTRSSM_PANEL_OBSERVATION ? a.src[0][1] : a.src[0][2];
  const float* pv = k == MTRSSM_PANEL_PRIOR ? a.src[1][0] : k == MTRSSM_PANEL_OBSERVATION ? a.src[1][1] : a.src[1][2];
  return m ? pv : pa;
}

// The colour of source element (sy, sx) of modality m (0 audio, 1 vision) in a column of kind `kind`.
__device__ __forceinline__ uint32_t cell_colour(const PanelArgs& a, const FrameState& fs, int m, int kind, int sy, int sx, const uint32_t* lut) {
  const int64_t at = (m ? fs.base[1] : fs.base[0]) + (int64_t)sy * (m ? a.W[1] : a.W[0]) + sx;
  const int plane = m ? a.plane[1] : a.plane[0];
  if (kind == MTRSSM_PANEL_ERROR) {
    const float* p = frames_of(a, m, MTRSSM_PANEL_PRIOR) + at;
    const float* o = frames_of(a, m, MTRSSM_PANEL_OBSERVATION) + at;
    float e = fabsf(to_unit(p[0]) - to_unit(o[0]));
    if (m == 1 && a.C[1] == 3) {
      const float e1 = fabsf(to_unit(p[plane]) - to_unit(o[plane]));
      const float e2 = fabsf(to_unit(p[2 * plane]) - to_unit(o[2 * plane]));
      e = ((e + e1) + e2) / 3.0f;
    }
    return magma_of(e, lut);
  }
  if (kind == MTRSSM_PANEL_OBSERVATION && a.blank_unseen && !((fs.code >> m) & 1)) return 0u;
  const float* v = frames_of(a, m, kind) + at;
  const float x = to_unit(v[0]);
  if (m == 0) return audio_colour(x, lut);
  const uint32_t r = (uint32_t)(int)(x * 255.0f);
  if (a.C[1] == 1) return r * 0x010101u;
  const uint32_t g = (uint32_t)(int)(to_unit(v[plane]) * 255.0f);
  const uint32_t b = (uint32_t)(int)(to_unit(v[2 * plane]) * 255.0f);
  return r | (g << 8) | (b << 16);
}

__global__ __launch_bounds__(kThreads) void episode_panel_kernel(PanelArgs a) {
  __shared__ uint32_t lut[256];
  for (int i = threadIdx.x; i < 256; i += kThreads) lut[i] = (uint32_t)kMagma[i][0] | ((uint32_t)kMagma[i][1] << 8) | ((uint32_t)kMagma[i][2] << 16);
  __syncthreads();
  const int64_t frame_pixels = (int64_t)a.Hc * a.Wc;
  const int64_t units = (a.pixels + 3) >> 2;
  const int pitch = a.cw + a.gap;
  const int box_h = 7 * a.label;
  for (int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x; u < units; u += (int64_t)gridDim.x * kThreads) {
    const int64_t p0 = u << 2;
    int f = (int)(p0 / frame_pixels);
    const int rem = (int)(p0 - (int64_t)f * frame_pixels);
    int y = rem / a.Wc, x = rem - y * a.Wc;
    const int count = a.pixels - p0 < 4 ? (int)(a.pixels - p0) : 4;
    FrameState fs = frame_state(a, f);
    RowState rs = row_state(a, y);
    int last_j = -1, last_sx = -1;  // the source element the previous pixel showed, and its colour
    uint32_t last = 0u;
    uint32_t px[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (k < count) {
        uint32_t c = 0u;
        if (fs.dead) {
          c = 0u;
        } else if (y < box_h && x < fs.box_w) {  // the frame number, drawn last: a box of 7 x (4 digits + 1) font pixels
          const int fy = div_small(y, a.inv_label, a.label) - 1, fx = div_small(x, a.inv_label, a.label) - 1;
          if (fy >= 0 && fy < 5 && fx >= 0 && (fx & 3) != 3 && (fx >> 2) < fs.digits) {
            int v = fs.value;
            for (int i = fs.digits - 1 - (fx >> 2); i > 0; --i) v /= 10;
            if ((kFont[v % 10] >> (14 - (3 * fy + (fx & 3)))) & 1) c = kWhite;
          }
        } else if (rs.band == 2) {
          c = fs.bar;
        } else if (rs.band == 3) {
          c = kGapColour;
        } else {
          int j = 0, xr = x;
          while (xr >= pitch) { xr -= pitch; ++j; }  // (at most 3 steps)
          const int m = rs.band;
          if (xr >= a.cw) {
            c = kGapColour;
          } else if (xr < (m ? a.W[1] : a.W[0]) * a.scale) {
            const int sx = div_small(xr, a.inv_scale, a.scale);
            if (j != last_j || sx != last_sx) {
              const int kind = j == 0 ? a.columns[0] : j == 1 ? a.columns[1] : j == 2 ? a.columns[2] : a.columns[3];
              last = cell_colour(a, fs, m, kind, rs.sy, sx, lut);
              last_j = j;
              last_sx = sx;
            }
            c = last;
          }  // (else: the cell's zero padding right of a narrower frame)
        }
        px[k] = c;
        if (++x == a.Wc) {
          x = 0;
          last_j = -1;
          if (++y == a.Hc) {
            y = 0;
            ++f;
            if (k + 1 < count) fs = frame_state(a, f);
          }
          rs = row_state(a, y);
        }
      }
    }
    const uint32_t d0 = px[0] | (px[1] << 24), d1 = (px[1] >> 8) | (px[2] << 16), d2 = (px[2] >> 16) | (px[3] << 8);
    uint32_t* o = reinterpret_cast<uint32_t*>(a.out) + 3 * u;
    if (count == 4) {
      o[0] = d0;
      o[1] = d1;
      o[2] = d2;
    } else {  // the video's last 1 .. 3 pixels: whole dwords while they fit, then the final 1 .. 3 bytes one by one
      const int bytes = 3 * count, whole = bytes >> 2;  // 3, 6 or 9 bytes: 0, 1 or 2 whole dwords
      if (whole > 0) o[0] = d0;
      if (whole > 1) o[1] = d1;
      const uint32_t rest = whole == 0 ? d0 : whole == 1 ? d1 : d2;
      unsigned char* tail = a.out + 12 * u + 4 * whole;
      for (int i = 0; i < (bytes & 3); ++i) tail[i] = (unsigned char)(rest >> (8 * i));
    }
  }
}

uint32_t reciprocal(int d) { return d <= 1 ? 0u : (uint32_t)(((uint64_t)1 << 32) / (uint64_t)d + 1); }

// Canvas size of a geometry, or false (with the error set).
bool canvas_of(const MtrssmPanelGeom* g, const char* who, int32_t* Hc, int32_t* Wc, int64_t* bytes) {
  if (!g) { set_error("%s: null geometry", who); return false; }
  if (g->N < 1 || g->T < 1 || g->Ca < 1 || g->Ha < 1 || g->Wa < 1 || g->Hv < 1 || g->Wv < 1) {
    set_error("%s: N, T and the frame sizes must be positive (got N %d T %d audio %dx%dx%d vision %dx%dx%d)", who, g->N, g->T, g->Ca, g->Ha, g->Wa,
              g->Cv, g->Hv, g->Wv);
    return false;
  }
  if (g->Cv != 1 && g->Cv != 3) { set_error("%s: vision frames have 1 or 3 channels (got %d)", who, g->Cv); return false; }
  if (g->scale < 1 || g->scale > kMaxScale || g->gap < 0 || g->gap > kMaxGap || g->bar < 0 || g->bar > kMaxBar || g->label < 0 ||
      g->label > kMaxLabel) {
    set_error("%s: need 1 <= scale <= %d, 0 <= gap <= %d, 0 <= bar <= %d, 0 <= label <= %d (got %d %d %d %d)", who, kMaxScale, kMaxGap, kMaxBar,
              kMaxLabel, g->scale, g->gap, g->bar, g->label);
    return false;
  }
  if (g->n_columns < 1 || g->n_columns > 4) { set_error("%s: 1 .. 4 columns (got %d)", who, g->n_columns); return false; }
  for (int j = 0; j < g->n_columns; ++j) {
    if (g->columns[j] < 0 || g->columns[j] > MTRSSM_PANEL_ERROR) { set_error("%s: column %d has kind %d, not 0 .. 3", who, j, g->columns[j]); return false; }
    for (int i = 0; i < j; ++i)
      if (g->columns[i] == g->columns[j]) { set_error("%s: column kind %d is given twice", who, g->columns[j]); return false; }
  }
  if (g->blank_unseen != 0 && g->blank_unseen != 1) { set_error("%s: blank_unseen is 0 or 1 (got %d)", who, g->blank_unseen); return false; }
  if (g->frame0 < 0 || (int64_t)g->frame0 + g->T > INT32_MAX) { set_error("%s: need 0 <= frame0 and frame0 + T < 2^31 (got %d)", who, g->frame0); return false; }
  const int64_t wmax = g->Wv > g->Wa ? g->Wv : g->Wa;
  const int64_t cw = wmax * g->scale;
  const int64_t w = g->n_columns * cw + (g->n_columns - 1) * (int64_t)g->gap;
  const int64_t h = (int64_t)g->bar + (int64_t)g->Hv * g->scale + g->gap + (int64_t)g->Ha * g->scale;
  if (w > kMaxCanvas || h > kMaxCanvas) { set_error("%s: the canvas is %lld x %lld, at most %d each way", who, (long long)h, (long long)w, kMaxCanvas); return false; }
  const int64_t frames = (int64_t)g->N * g->T;
  const int64_t ea = (int64_t)g->Ca * g->Ha * g->Wa, ev = (int64_t)g->Cv * g->Hv * g->Wv;
  if (frames > INT32_MAX || frames > (((int64_t)1 << 60) / (h * w * 3)) || frames > (((int64_t)1 << 60) / (ea > ev ? ea : ev))) {
    set_error("%s: N * T = %lld frames are too many", who, (long long)frames);
    return false;
  }
  if (Hc) *Hc = (int32_t)h;
  if (Wc) *Wc = (int32_t)w;
  if (bytes) *bytes = frames * h * w * 3;
  return true;
}

}  // namespace

int64_t episode_panel_bytes(const MtrssmPanelGeom* g, int32_t* Hc, int32_t* Wc) {
  int64_t bytes = 0;
  if (!canvas_of(g, "episode_panel_bytes", Hc, Wc, &bytes)) return MTRSSM_EINVAL;
  return bytes;
}

int episode_panel_launch(const MtrssmPanelGeom* g, const float* obs_a, const float* post_a, const float* prior_a, const float* obs_v,
                         const float* post_v, const float* prior_v, const int32_t* codes, const int32_t* valid, const int32_t* context,
                         unsigned char* out, hipStream_t s) {
  int32_t Hc = 0, Wc = 0;
  int64_t bytes = 0;
  if (!canvas_of(g, "episode_panel", &Hc, &Wc, &bytes)) return MTRSSM_EINVAL;
  if (!context || !out) { set_error("episode_panel: null context or out"); return MTRSSM_EINVAL; }
  bool need[3] = {false, false, false};
  for (int j = 0; j < g->n_columns; ++j) {
    if (g->columns[j] == MTRSSM_PANEL_ERROR) need[MTRSSM_PANEL_PRIOR] = need[MTRSSM_PANEL_OBSERVATION] = true;
    else need[g->columns[j]] = true;
  }
  PanelArgs a;
  const float* given[2][3] = {{prior_a, obs_a, post_a}, {prior_v, obs_v, post_v}};
  static const char* const kNames[3] = {"prior", "observation", "posterior"};
  uintptr_t low = (uintptr_t)out | (uintptr_t)codes | (uintptr_t)valid | (uintptr_t)context;
  for (int m = 0; m < 2; ++m) {
    for (int k = 0; k < 3; ++k) {
      if (need[k] && !given[m][k]) { set_error("episode_panel: the columns need the %s frames of both modalities (null)", kNames[k]); return MTRSSM_EINVAL; }
      a.src[m][k] = given[m][k];
      low |= (uintptr_t)given[m][k];
    }
  }
  if (low & 3) { set_error("episode_panel: buffers must be 4-byte aligned"); return MTRSSM_EINVAL; }
  a.codes = codes; a.valid = valid; a.context = context; a.out = out;
  a.pixels = bytes / 3;
  a.C[0] = g->Ca; a.H[0] = g->Ha; a.W[0] = g->Wa;
  a.C[1] = g->Cv; a.H[1] = g->Hv; a.W[1] = g->Wv;
  for (int m = 0; m < 2; ++m) {
    a.plane[m] = a.H[m] * a.W[m];
    a.frame_elems[m] = (int64_t)a.C[m] * a.plane[m];
  }
  a.T = g->T; a.Hc = Hc; a.Wc = Wc;
  a.cw = (g->Wv > g->Wa ? g->Wv : g->Wa) * g->scale;
  a.hv = g->Hv * g->scale;
  a.scale = g->scale; a.gap = g->gap; a.bar = g->bar; a.label = g->label; a.frame0 = g->frame0;
  a.n_columns = g->n_columns; a.blank_unseen = g->blank_unseen;
  for (int j = 0; j < 4; ++j) a.columns[j] = j < g->n_columns ? g->columns[j] : 0;
  a.inv_scale = reciprocal(g->scale);
  a.inv_label = reciprocal(g->label);
  const int64_t units = (a.pixels + 3) / 4;
  const int64_t blocks = (units + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(episode_panel_kernel, dim3((unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks)), dim3(kThreads), 0, s, a);
  set_last_kernel("mtrssm::episode_panel_kernel");
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("episode_panel launch failed: %s", hipGetErrorString(e)); return MTRSSM_ELAUNCH; }
  return MTRSSM_OK;
}

}  // namespace mtrssm
