// The forward plans of libsketchedit_hip.so: the layer tables of netM / netG, the launcher of one gated conv, the plans of the
// two networks with the attention driver, and how a forward's batch is split into passes and its workspace into arenas.
//
// Layer tables restate the reference constructors
//   DeepFillC2Generator.__init__  /root/reference/models/networks/editline_g.py:44-100
//   MDGenerator.__init__          /root/reference/models/networks/editline2_g.py:18-43
// and the plans restate the forward methods (editline_g.py:119-221, editline2_g.py:59-94,
// editline2_model.py:128-133,338-370).
#include "se_host.h"

#include <numeric>

using namespace se;

namespace {

#define ENC(p)                                                                                    \
  {p "2_downsample", 24, 96, 3, 2, 1, ACT_ELU, 0}, {p "3", 48, 96, 3, 1, 1, ACT_ELU, 0},          \
      {p "4_downsample", 48, 192, 3, 2, 1, ACT_ELU, 0}, {p "5", 96, 192, 3, 1, 1, ACT_ELU, 0},    \
      {p "6", 96, 192, 3, 1, 1, ACT_ELU, 0}, {p "7_atrous", 96, 192, 3, 1, 2, ACT_ELU, 0},        \
      {p "8_atrous", 96, 192, 3, 1, 4, ACT_ELU, 0}, {p "9_atrous", 96, 192, 3, 1, 8, ACT_ELU, 0}, \
      {p "10_atrous", 96, 192, 3, 1, 16, ACT_ELU, 0}
#define DEC(p, c11in, c17out)                                                                        \
  {p "11", c11in, 192, 3, 1, 1, ACT_ELU, 0}, {p "12", 96, 192, 3, 1, 1, ACT_ELU, 0},                 \
      {p "13_upsample_conv", 96, 96, 3, 1, 1, ACT_ELU, 1}, {p "14", 48, 96, 3, 1, 1, ACT_ELU, 0},    \
      {p "15_upsample_conv", 48, 48, 3, 1, 1, ACT_ELU, 1}, {p "16", 24, 24, 3, 1, 1, ACT_ELU, 0},    \
      {p "17", 12, c17out, 3, 1, 1, ACT_NONE, 0}

}  // namespace

namespace se {

const LayerDef G_LAYERS[] = {
    {"conv1", 5, 48, 5, 1, 1, ACT_ELU, 0}, ENC("conv"), DEC("conv", 192, 3),
    {"wconv1", 5, 48, 5, 1, 1, ACT_ELU, 0}, ENC("wconv"),
    {"xconv1", 3, 48, 5, 1, 1, ACT_ELU, 0},
    {"xconv2_downsample", 24, 48, 3, 2, 1, ACT_ELU, 0}, {"xconv3", 24, 96, 3, 1, 1, ACT_ELU, 0},
    {"xconv4_downsample", 48, 96, 3, 2, 1, ACT_ELU, 0}, {"xconv5", 48, 192, 3, 1, 1, ACT_ELU, 0},
    {"xconv6", 96, 192, 3, 1, 1, ACT_ELU, 0}, {"xconv7_atrous", 96, 192, 3, 1, 2, ACT_ELU, 0},
    {"xconv8_atrous", 96, 192, 3, 1, 4, ACT_ELU, 0}, {"xconv9_atrous", 96, 192, 3, 1, 8, ACT_ELU, 0},
    {"xconv10_atrous", 96, 192, 3, 1, 16, ACT_ELU, 0},
    {"pmconv1", 3, 48, 5, 1, 1, ACT_ELU, 0},
    {"pmconv2_downsample", 24, 48, 3, 2, 1, ACT_ELU, 0}, {"pmconv3", 24, 96, 3, 1, 1, ACT_ELU, 0},
    {"pmconv4_downsample", 48, 192, 3, 2, 1, ACT_ELU, 0}, {"pmconv5", 96, 192, 3, 1, 1, ACT_ELU, 0},
    {"pmconv6", 96, 192, 3, 1, 1, ACT_RELU, 0}, {"pmconv9", 96, 192, 3, 1, 1, ACT_ELU, 0},
    {"pmconv10", 96, 192, 3, 1, 1, ACT_ELU, 0},
    DEC("allconv", 192, 3),
};
const LayerDef M_LAYERS[] = {
    {"conv1", 4, 48, 5, 1, 1, ACT_ELU, 0}, ENC("conv"), DEC("conv", 96, 3), DEC("conv_mask_", 96, 1),
};
const int NG = sizeof(G_LAYERS) / sizeof(LayerDef), NM = sizeof(M_LAYERS) / sizeof(LayerDef);

}  // namespace se

namespace {

// ---- launching one gated conv ---------------------------------------------------------------------------------------
// choose_form (se_dispatch.h) decides the kernel form of a call; run_gconv below switches into one launcher per family, which
// fills that family's params and launch cost and launches.  A launcher decides nothing: what it reads of `ch` is the choice.
struct ConvLaunch {       // one call: where it runs, the layer, the sources (src1: a tensor, a vector or null), the sizes
  se_ctx* c;
  const Layer& L; const LayerDef& d; const LayerFacts& f;
  const float* src0; int C0; const float* src1; int C1, src1_vec; float* dst;
  int B, Hin, Win, Ho, Wo, pad;
  bool bf;
  double alg(int taps) const { return 2.0 * (double)B * Ho * Wo * d.cout * d.cin * taps; }       // the layer's cost as the reference defines it

  // a Winograd launch on tiles of 2 rows x `tcols` columns at dilation `dil` (no second source, no folded bias: the caller sets those)
  WinoParams wino_params(const float* upk, const float* bias, int dil, int tcols) const {
    WinoParams wp;
    memset(&wp, 0, sizeof wp);
    wp.src = src0; wp.upk = upk; wp.bias = bias; wp.dst = dst;
    wp.B = B; wp.h = Hin; wp.w = Win; wp.d = dil; wp.th = Hin / 2; wp.tw = Win / tcols;
    wp.total_tiles = B * wp.th * wp.tw; wp.act = d.act;
    wp.xcd = xcd_remap_enabled();
    udiv_magic_host((unsigned)(wp.th * wp.tw), &wp.div_tpi_m, &wp.div_tpi_l);
    udiv_magic_host((unsigned)wp.tw, &wp.div_tw_m, &wp.div_tw_l);
    udiv_magic_host((unsigned)wp.d, &wp.div_d_m, &wp.div_d_l);
    return wp;
  }
  // 96 (+ 96) -> 192 and 48 -> 192: F(2x2,3x3), 16 of 36 products (se_wino.hip); hybrid F(2,3) x F(4,3) on 2x4 tiles, 24 of 72
  // (se_wino24.hip).  Folded vector source: half the positions' K, only the first source's half executed (311 -> 170 us at 256x256 B=32)
  int launch_form_wino(const Choice& ch) const {
    const double alg3x3 = alg(9);
    if (ch.form == F_WINO24_C48) {       // xconv5: 2 chunks per position, the second half empty
      const WinoParams wp = wino_params(L.d_u24, L.d_ub24, d.rate, 4);
      set_launch_cost(alg3x3, 4.0 * ((double)B * Hin * Win * 48 + (double)B * Hin * Win * 96), d.name, alg3x3 * 24.0 / 72.0);
      HIPCHK(c, launch_wino24_c48(wp, c->st));
      return 0;
    }
    const bool folded = ch.fold, f43 = ch.form == F_WINO24;
    if (folded) HIPCHK(c, launch_vecbias(L.d_wv, src1, c->vbias_ws, B, 96, c->st));
    const float* s1 = folded ? nullptr : src1;
    WinoParams wp = f43 ? wino_params(s1 ? L.d_u24b : L.d_u24, L.d_ub24, d.rate, 4) : wino_params(folded ? L.d_u1 : L.d_u, L.d_b, d.rate, 2);
    wp.src1 = s1; wp.src1_vec = folded ? 0 : src1_vec; wp.vbias = folded ? c->vbias_ws : nullptr;
    if ((double)B * Hin * Win * 384.0 >= 2147483648.0) return fail(c, "layer %s: tensor exceeds 2^31 bytes", d.name);
    set_launch_cost(alg3x3, 4.0 * 2.0 * (double)B * Hin * Win * 96, d.name,
                    f43 ? alg3x3 * 24.0 / 72.0 * (folded ? 0.5 : 1.0) : alg3x3 * 16.0 / 36.0 * (folded ? 0.5 : 1.0));
    HIPCHK(c, f43 ? launch_wino24(wp, c->st) : launch_wino(wp, c->st));
    return 0;
  }
  // 48 -> 96, and 24 -> 96 with one chunk per position (se_wino48.hip): 16 of 36 products
  int launch_form_wino48(const Choice& ch) const {
    const WinoParams wp = wino_params(L.d_u, L.d_ub, d.rate, 2);
    const bool c24 = ch.form == F_WINO48_C24;
    set_launch_cost(alg(9), c24 ? 4.0 * ((double)B * Hin * Win * 24 + (double)B * Hin * Win * 48) : 4.0 * 2.0 * (double)B * Hin * Win * 48, d.name,
                    alg(9) * 16.0 / 36.0);
    HIPCHK(c, c24 ? launch_wino48_c24(wp, c->st) : launch_wino48(wp, c->st));
    return 0;
  }
  // 3x3 stride 2, 48 -> 96 / 192: polyphase F(2,2), 25 of 36 products (se_s2poly.hip; 75 k-halves executed, 76 staged); a
  // 192-row layer as two 96-row halves that both transform the source
  int launch_form_s2poly(const Choice&) const {
    const int halves = d.cout / 96;
    WinoParams wp = wino_params(L.d_s2p, L.d_s2pb, 1, 2);
    wp.th = Hin / 4; wp.tw = Win / 4; wp.total_tiles = B * wp.th * wp.tw;
    udiv_magic_host((unsigned)(wp.th * wp.tw), &wp.div_tpi_m, &wp.div_tpi_l);
    udiv_magic_host((unsigned)wp.tw, &wp.div_tw_m, &wp.div_tw_l);
    set_launch_cost(alg(9), 4.0 * ((double)halves * B * Hin * Win * 48 + (double)B * Ho * Wo * (d.cout / 2)), d.name, alg(9) * 25.0 / 36.0);
    HIPCHK(c, launch_s2poly48(wp, halves, c->st));
    return 0;
  }
  // gen_deconv 96 -> 96 and 48 -> 48: F(2x2,2x2) on the sub-pixel classes, 9 of 36 products (se_wino_up.hip, se_wino_up48.hip;
  // 48: in the K pairing of the 48-channel kernels, 28 k-halves executed for 27 of work)
  int launch_form_winoup(const Choice& ch) const {
    const WinoParams wp = wino_params(L.d_u, L.d_ub, 1, 2);
    if (ch.form == F_WINOUP) {
      set_launch_cost(alg(9), 4.0 * ((double)B * Hin * Win * 96 + (double)B * Ho * Wo * 48), d.name, alg(9) * 9.0 / 36.0);
      HIPCHK(c, launch_winoup(wp, c->st));
      return 0;
    }
    set_launch_cost(alg(9), 4.0 * ((double)B * Hin * Win * 48 + (double)B * Ho * Wo * 24), d.name, alg(9) * 9.0 / 36.0 * 28.0 / 27.0);
    HIPCHK(c, launch_winoup48(wp, c->st));
    return 0;
  }

  // what every raw-tile launch of the narrow layers starts from: `trows` output rows x 16 columns per tile
  RTileParams rtile_params(const float* wpk, int trows) const {
    RTileParams p;
    memset(&p, 0, sizeof p);
    p.src = src0; p.wpk = wpk; p.bias = L.d_b; p.dst = dst;
    p.B = B; p.Hin = Hin; p.Win = Win; p.C = C0; p.OH = Ho; p.OW = Wo;
    p.G = bf ? (f.G + 7) & ~7 : f.G; p.NP = f.NP;
    p.ty = (Hin + trows - 1) / trows; p.tx = (Win + 15) / 16;
    p.act = d.act; p.bf16 = bf ? 1 : 0; p.xcd = xcd_remap_enabled();
    return p;
  }
  // 24 -> 24 3x3: F(2,3) along x on the raw tile, 160 instead of 224 MFMAs per wave, or two-dimensional, 96 (se_rtilew.hip)
  int launch_form_rtilew(const Choice& ch) const {
    const bool two_d = ch.form == F_RTILEW2;
    RTileParams p = rtile_params(two_d ? L.d_wx2 : L.d_wx, 16);       // blocks of 16 x 16 outputs
    udiv_magic_host((unsigned)(p.ty * p.tx), &p.div_cg_m, &p.div_cg_l);      // (reused fields: blk / (ty * tx), t2 / tx)
    udiv_magic_host((unsigned)p.tx, &p.div_rw_m, &p.div_rw_l);
    set_launch_cost(alg(9), 4.0 * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name,
                    (double)B * p.ty * p.tx * 8.0 * (two_d ? 96.0 : 160.0) * 2048.0);       // MFMAs of 16x16x4 per wave and block
    HIPCHK(c, two_d ? launch_rtilew2(p, c->st) : launch_rtilew(p, c->st));
    return 0;
  }
  // dense-K form of the 5x5 first layers (fp32), direct or F(2,5) along x (rtile_dense5w_kernel: 6 positions x ceil(5 Cd / 4)
  // k-steps per 2 outputs).  The kernel addresses its source with 32-bit byte offsets: a batch beyond that range is run as
  // sub-launches of the SAME kernel form over image ranges (switching to the channel-padded kernel would change the
  // summation order, i.e. the bit-identity of an image's result across batch compositions within one execution mode).
  int launch_form_rtile_dense5(const Choice& ch) const {
    const bool along_x = ch.form == F_RTILE_DENSE5W;
    const long long per_img = (long long)Hin * Win * C0 * 4;
    const long long lim = addr_limit();       // (SE_TEST_OFFSET_LIMIT, a test aid: a smaller byte range forces the sub-launches)
    const int bmax = (int)std::max<long long>(1, (lim - 1) / per_img);
    for (int b0 = 0; b0 < B; b0 += bmax) {
      const int nb = std::min(bmax, B - b0);
      RTileParams p = rtile_params(along_x ? L.d_wdw : L.d_wd, 8);
      p.src = src0 + (size_t)b0 * Hin * Win * C0; p.dst = dst + (size_t)b0 * Ho * Wo * f.G; p.B = nb;
      p.dense = along_x ? f.dense + 100 : f.dense; p.nch = f.nchd;
      const double algn = 2.0 * (double)nb * Ho * Wo * d.cout * d.cin * 25;
      set_launch_cost(algn, 4.0 * ((double)nb * Hin * Win * d.cin + (double)nb * Ho * Wo * (d.cout / 2)), d.name,
                      along_x ? (double)nb * p.ty * p.tx * 4.0 * (6.0 * ((5 * f.dense + 3) / 4) * 3.0) * 2048.0
                              : 2.0 * (double)nb * Hin * Win * 48.0 * (4.0 * ((25 * f.dense + 3) / 4)));       // ceil(K / 4) k-steps of 4
      HIPCHK(c, launch_rtile(p, c->st));
    }
    return 0;
  }
  // the raw-tile kernel on the direct image (se_rtile.hip), fp32 and bf16; bf16 pair-of-taps form of the 5x5 first layers
  int launch_form_rtile(const Choice& ch) const {
    const int es = bf ? 2 : 4, TR = rtile_rows(bf);
    RTileParams p = rtile_params(ch.form == F_RTILE_D4 ? L.d_w16d : L.direct[bf], TR);
    p.pad = pad;
    if (ch.form == F_RTILE_D4) {
      p.CG = 1; p.T = 25; p.KW = 5; p.nch = 2; p.dense = 204;
      p.RH = 32 + 4; p.RW = 21;                     // one column more than the halo: the sixth tap of a pair row
      p.raw_bytes = (p.RH * p.RW * 8 + 1023) & ~1023;
      udiv_magic_host(1u, &p.div_cg_m, &p.div_cg_l);
      set_launch_cost(alg(25), 2.0 * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name, 2.0 * (double)B * Hin * Win * 48.0 * 128.0);
    } else {
      const int KW = d.up ? 2 : d.k, CG = f.CG[bf], nch = f.nch[bf];
      p.CG = CG; p.T = f.T; p.KW = KW; p.nch = nch; p.up2 = d.up ? 1 : 0;
      p.RH = TR + KW - 1; p.RW = 16 + KW - 1;
      p.raw_bytes = (p.RH * p.RW * C0 * es + 1023) & ~1023;
      p.magicCG = (65536 + CG - 1) / CG; p.magicKW = 256 / KW + 1;        // (choose_form verified both on the ranges used)
      udiv_magic_host((unsigned)(C0 * es / 16), &p.div_cg_m, &p.div_cg_l);
      set_launch_cost(alg(d.k * d.k), (double)es * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name,
                      2.0 * (double)B * Hin * Win * (d.up ? 4.0 : 1.0) * f.NP * (nch * (bf ? 64.0 : 32.0)));
    }
    udiv_magic_host((unsigned)p.RW, &p.div_rw_m, &p.div_rw_l);
    HIPCHK(c, launch_rtile(p, c->st));
    return 0;
  }

  // bf16, 96 -> 192 3x3 stride 1 on 8 x 16 raw tiles of the polyphase sub-images (se_rconv16.hip).  dual: sub-images of 8 x 8
  // (dilation 16 at 128 x 128, 8 at 64 x 64), two phases share a tile.  fold (conv11 of netG): the spatially constant second
  // source folded into a bias table, the layer on the first source alone
  int launch_form_rconv16(const Choice& ch) const {
    if (ch.fold) HIPCHK(c, launch_vecbias(L.d_wv16, c->vec32, c->vbias_ws, B, 96, c->st, 1));
    RConvParams rp;
    memset(&rp, 0, sizeof rp);
    rp.dual = ch.form == F_RCONV16_DUAL;
    rp.src = src0; rp.wpk = L.d_w16s; rp.bias = L.d_b; rp.dst = dst; rp.vbias = ch.fold ? c->vbias_ws : nullptr;
    rp.B = B; rp.h = Hin; rp.w = Win; rp.d = d.rate; rp.hs = Hin / d.rate; rp.ws = Win / d.rate;
    rp.ty = (rp.hs + 7) / 8; rp.tx = (rp.ws + 15) / 16;
    rp.act = d.act; rp.xcd = xcd_remap_enabled();
    set_launch_cost(alg(9), 2.0 * 2.0 * (double)B * Hin * Win * 96, d.name, 2.0 * (double)B * Hin * Win * 192.0 * 864.0);
    HIPCHK(c, launch_rconv16(rp, c->st));
    return 0;
  }
  // bf16, the 96-row layers (3x3 48/24 -> 96 at stride 1, 24 -> 96 at stride 2, gen_deconv 96 -> 96): se_rconv96.hip
  int launch_form_rconv96(const Choice&) const {
    RConv96Params rp;
    memset(&rp, 0, sizeof rp);
    rp.src = src0; rp.wpk = L.d_w96; rp.bias = L.d_b; rp.dst = dst;
    rp.B = B; rp.h = Hin; rp.w = Win; rp.CG = C0 / 8;
    rp.stride = d.stride; rp.oh = Ho; rp.ow = Wo;
    rp.ty = ((d.stride == 2 ? Ho : Hin) + 15) / 16; rp.tx = ((d.stride == 2 ? Wo : Win) + 15) / 16;
    rp.up2 = d.up ? 1 : 0; rp.act = d.act; rp.xcd = xcd_remap_enabled();
    const int T = d.up ? 4 : 9, nstep = (T * rp.CG + 3) / 4;
    set_launch_cost(alg(9), 2.0 * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * 48), d.name,
                    2.0 * (double)B * (d.stride == 2 ? (double)Ho * Wo : (double)Hin * Win) * (d.up ? 4.0 : 1.0) * 96.0 * (nstep * 32.0));
    HIPCHK(c, launch_rconv96(rp, c->st));
    return 0;
  }

  // the direct gather-GEMM (se_gconv.hip) on the image of one precision: the fallback of every gated conv
  int launch_form_gather(const Choice&) const {
    const int es = bf ? 2 : 4, gran = bf ? 8 : 4, CG = f.CG[bf], nch = f.nch[bf], KW = d.up ? 2 : d.k;
    GConvParams p;
    memset(&p, 0, sizeof p);
    p.bf16 = bf ? 1 : 0;
    p.src0 = src0; p.src1 = src1 ? src1 : src0; p.wpk = L.direct[bf]; p.bias = L.d_b; p.dst = dst; p.zeros = c->zeros;
    p.B = B; p.Hin = Hin; p.Win = Win; p.Ho = d.up ? Hin : Ho; p.Wo = d.up ? Win : Wo;   // up2: rows walk the source grid
    p.up2 = d.up ? 1 : 0; p.OH = Ho; p.OW = Wo;
    p.C0 = C0; p.C1 = C1 ? C1 : C0; p.C0g = C0 / gran; p.CG = CG;
    p.T = f.T; p.KW = KW; p.stride = d.stride; p.dil = d.rate; p.pad = pad;
    p.magicCG = (65536 + CG - 1) / CG; p.magicKW = 256 / KW + 1; p.magicKH = f.T / KW;
    if (!magic_cg_ok(CG, nch)) return fail(c, "layer %s: magic division check failed", d.name);
    if (!magic_kw_ok(KW, f.T)) return fail(c, "layer %s: magic tap division check failed", d.name);
    const int Gs = bf ? (f.G + 7) & ~7 : f.G;      // stored channel stride of the output
    // 32-bit byte offsets (sentinel 0x80000000): source and destination below 2^31 BYTES
    if ((double)B * Hin * Win * (C0 > C1 ? C0 : C1) * es >= 2147483648.0 || (double)B * Ho * Wo * Gs * es >= 2147483648.0)
      return fail(c, "layer %s: a tensor of this launch exceeds 2^31 bytes (32-bit byte offsets) -- split the batch", d.name);
    for (int j = 0; j < p.magicKH; ++j) p.rep |= 1u << (j * KW);
    udiv_magic_host((unsigned)(p.Ho * p.Wo), &p.div_hw_m, &p.div_hw_l);
    udiv_magic_host((unsigned)p.Wo, &p.div_w_m, &p.div_w_l);
    p.Hlim = Hin; p.Wlim = Win;
    p.src1_vec = src1_vec; p.nch = nch; p.G = Gs; p.act = d.act; p.total_pix = B * p.Ho * p.Wo;
    p.xcd = xcd_remap_enabled();
    p.np_full = f.NP; p.nf_full = f.NP / 32; p.small_grid = c->low_latency ? 1 : 0;
    // cost: algorithmic as the reference defines the layer (3x3 on the upsampled grid for gen_deconv); executed: the packed K
    // (channels padded to granules, taps x channels padded to whole chunks) and row (NP) sizes the MFMAs really run over; the
    // sub-pixel form of gen_deconv runs 4 classes x 4 taps instead of 9 taps on the upsampled grid
    set_launch_cost(alg(d.k * d.k), (double)es * ((double)B * Hin * Win * d.cin + (double)B * Ho * Wo * (d.cout / 2)), d.name,
                    2.0 * (double)B * p.Ho * p.Wo * (d.up ? 4.0 : 1.0) * f.NP * (nch * (bf ? 64.0 : 32.0)));
    HIPCHK(c, launch_gconv(f.cfg, p, c->st));
    return 0;
  }
};

}  // namespace

namespace se {

int run_gconv(se_ctx* c, const Layer& L, const float* src0, int C0, const float* src1, int C1, int src1_vec, float* dst,
              int B, int Hin, int Win) {
  const LayerDef& d = L.def;
  const LayerFacts& f = L.facts;
  const ConvShape sh = conv_shape(d, Hin, Win);
  const bool bf = c->bf16;
  if (!L.packed) return fail(c, "layer %s: weights not loaded", d.name);
  if (bf && !L.direct[1]) return fail(c, "layer %s: no bf16 weight image", d.name);
  if (bf && (C0 + C1) != f.CG[1] * 8) return fail(c, "layer %s: bf16 source channels %d+%d != packed %d", d.name, C0, C1, f.CG[1] * 8);
  if (!bf && (C0 + C1) != f.CG[0] * 4) return fail(c, "layer %s: source channels %d+%d != packed %d", d.name, C0, C1, f.CG[0] * 4);
  const ConvCall q = {d, f, B, Hin, Win, C0, C1, src1 ? (src1_vec ? SRC2_VECTOR : SRC2_TENSOR) : SRC2_NONE, bf, c->low_latency,
                      c->conservative, c->cur_net, c->vbias_ws && (!bf || c->vec32)};
  const Choice ch = choose_form(q);
  static bool said = false;
  if (ch.wino_range && !said) {
    said = true;
    fprintf(stderr, "sketchedit_hip: layer %s: %d x %dx%d x 96 floats exceed the Winograd kernel's 32-bit byte offsets; "
                    "using the direct kernel (about 2x slower) -- split the batch\n", d.name, B, Hin, Win);
  }
  const ConvLaunch a = {c, L, d, f, src0, C0, src1, C1, src1_vec, dst, B, Hin, Win, sh.Ho, sh.Wo, sh.pad, bf};
  switch (ch.form) {
    case F_WINO: case F_WINO24: case F_WINO24_C48: return a.launch_form_wino(ch);
    case F_WINO48: case F_WINO48_C24: return a.launch_form_wino48(ch);
    case F_WINOUP: case F_WINOUP48: return a.launch_form_winoup(ch);
    case F_RTILEW: case F_RTILEW2: return a.launch_form_rtilew(ch);
    case F_RTILE_DENSE5: case F_RTILE_DENSE5W: return a.launch_form_rtile_dense5(ch);
    case F_RTILE: case F_RTILE_D4: return a.launch_form_rtile(ch);
    case F_RCONV16: case F_RCONV16_DUAL: return a.launch_form_rconv16(ch);
    case F_RCONV96: return a.launch_form_rconv96(ch);
    case F_S2POLY48: return a.launch_form_s2poly(ch);
    case F_GATHER: return a.launch_form_gather(ch);
    case F_SMALL_CONV: break;      // (a raw layer has no gated image: refused above)
  }
  return fail(c, "layer %s: not a gated conv", d.name);
}

}  // namespace se

namespace {

// encoder: conv1 (5x5) .. conv10_atrous; returns conv10 output, optionally keeps conv9's
Act encoder(Plan& P, const std::string& p, Act& in, Act* keep9, Layer* first = nullptr) {
  Act x = first ? P.conv_layer(*first, in) : P.conv((p + "1").c_str(), in);
  x = P.conv((p + "2_downsample").c_str(), x);
  x = P.conv((p + "3").c_str(), x);
  x = P.conv((p + "4_downsample").c_str(), x);
  x = P.conv((p + "5").c_str(), x);
  x = P.conv((p + "6").c_str(), x);
  x = P.conv((p + "7_atrous").c_str(), x);
  x = P.conv((p + "8_atrous").c_str(), x);
  Act x9 = P.conv((p + "9_atrous").c_str(), x);
  Act x10 = P.conv((p + "10_atrous").c_str(), x9, keep9 == nullptr);
  if (keep9) *keep9 = x9;
  return x10;
}

// decoder conv11..conv16 (returns the 12-channel full-resolution activation feeding conv17)
Act decoder(Plan& P, const std::string& p, Act& in, const float* src1 = nullptr, int C1 = 0, int vec = 0) {
  Act x = P.conv((p + "11").c_str(), in, true, src1, C1, vec);
  x = P.conv((p + "12").c_str(), x);
  x = P.conv((p + "13_upsample_conv").c_str(), x);
  x = P.conv((p + "14").c_str(), x);
  x = P.conv((p + "15_upsample_conv").c_str(), x);
  x = P.conv((p + "16").c_str(), x);
  return x;
}

int small(Plan& P, const char* name, Act& in, int mode, float* out_nchw, float* hard, const float* img,
          const float* mask, float* xnow, float* composed, int no_mask_coarse, long packed_bs = 0,
          const unsigned char* lock = nullptr, bool raw_fine = false) {
  if (P.rc) return P.rc;
  se_ctx* c = P.c;
  if (!c->dry) {
    Layer& L = P.net.at(name);
    if (!L.packed) return P.rc = fail(c, "layer %s: weights not loaded", name);
    SmallConvParams sp;
    memset(&sp, 0, sizeof sp);
    sp.x = in.p; sp.w = L.direct[c->bf16]; sp.b = L.d_b; sp.B = P.B; sp.H = in.H; sp.W = in.W; sp.cout = L.def.cout;
    sp.bf16 = c->bf16 ? 1 : 0;
    sp.mode = mode; sp.out_nchw = out_nchw; sp.hard = hard; sp.img = img; sp.mask = mask; sp.xnow = xnow;
    sp.composed = composed; sp.no_mask_coarse = no_mask_coarse;
    if (mode == 3) { sp.rgb8 = c->rgb8; sp.m8 = c->m8; }
    if (mode == 3 && raw_fine && sp.rgb8) sp.raw_fine = 1;      // SE_FLAG_RAW_FINE: the kernel's RAW form
    if (mode == 0) sp.lock = lock;
    if (packed_bs) {      // SE_FLAG_PACKED_OUT: soft mask and composite live in one (B,4,H,W) buffer
      if (mode == 0) sp.out_bs = packed_bs;
      if (mode == 3) { sp.mask_bs = packed_bs; sp.comp_bs = packed_bs; }
    }
    set_launch_cost(2.0 * (double)P.B * in.H * in.W * L.def.cout * 108.0,
                    4.0 * (double)P.B * in.H * in.W * (12 + L.def.cout), L.def.name);
    hipError_t e = launch_small_conv(sp, c->st);
    if (e != hipSuccess) return P.rc = fail(c, "small conv %s: %s", name, hipGetErrorString(e));
  }
  P.free(in);
  return 0;
}

}  // namespace

namespace se {

// MDGenerator.forward, editline2_g.py:59-94.  lock (B,H,W) uint8 or null: the mask is 0 where it is non-zero
int plan_netM(se_ctx* c, const float* image, const float* sketch, float* mask_out, float* hard_out, float* maskim_out,
              int B, int H, int W, long packed_bs, const unsigned char* lock) {
  Plan P(c, c->M, B);
  c->cur_net = SE_NET_M;
  Act in = P.alloc(H, W, 4);
  if (P.rc) return P.rc;
  if (!c->dry) HIPCHK(c, c->bf16 ? launch_pack_m16(image, sketch, in.p, B, H, W, c->st) : launch_pack_m(image, sketch, in.p, B, H, W, c->st));
  Act x9;
  const bool want_img = maskim_out != nullptr;
  Act x10 = encoder(P, "conv", in, want_img ? &x9 : nullptr);
  if (want_img) {   // image decoder consumes conv9's output (quirk, editline2_g.py:76-77)
    Act d = decoder(P, "conv", x9);
    small(P, "conv17", d, 1, maskim_out, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
  }
  Act d = decoder(P, "conv_mask_", x10);
  small(P, "conv_mask_17", d, 0, mask_out, hard_out, nullptr, nullptr, nullptr, nullptr, 0, packed_bs, lock);
  return P.rc;
}

// DeepFillC2Generator.forward, editline_g.py:119-221.  The two encoders of stage 1 and the two branches of stage 2 are
// independent until their concat: in low-latency mode the second one of each pair runs on the side stream.
int plan_netG(se_ctx* c, const float* x, const float* x2, const float* mask, const float* mask2, const float* guide,
              float* coarse_out, float* fine_out, const float* soft_mask, float* composed_out, int B, int H, int W,
              int flags, long packed_bs) {
  Plan P(c, c->G, B);
  c->cur_net = SE_NET_G;
  const int joint = (flags & SE_FLAG_JOINT_TRAIN_INP) ? 1 : 0;
  // joint_train_inp: the style input is packed without its (zero) guide channel and wconv1 runs as a 4-channel conv
  Act cin = P.alloc(H, W, 8);
  P.ar = P.forked() ? &c->arena2 : P.home();        // the style branch's input lives in the style branch's arena
  Act sin = P.alloc(H, W, joint ? 4 : 8);
  P.ar = P.home();
  if (P.rc) return P.rc;
  if (!c->dry)
    HIPCHK(c, (c->bf16 ? launch_pack_g16 : launch_pack_g)(x, x2, mask, mask2, guide, cin.p, sin.p, B, H, W,
                                                          (flags & SE_FLAG_NO_MASK_CC) ? 1 : 0, joint, c->st));
  // ---- style branch :149-163 -> (B,96) pooled vector, consumed by conv11 as a second (spatially constant) source
  if (P.side_begin()) return 1;
  Act xs = encoder(P, "wconv", sin, nullptr, joint ? &c->wconv1_j4 : nullptr);
  // (in bf16 mode `part` / `vec32` hold fp32 values in twice the room they need; `vec` is the bf16 vector conv11 reads)
  Act part = P.alloc(1, COLREDUCE_SPLITS, 192), vec32 = P.alloc(1, 1, 192), vec = P.alloc(1, 1, 96);
  if (P.rc) return P.rc;
  if (!c->dry)
    HIPCHK(c, launch_colreduce(xs.p, part.p, c->bf16 ? vec32.p : vec.p, B, xs.H * xs.W, 96, (flags & SE_FLAG_POOL_MAX) ? 0 : 1,
                               c->st, c->bf16 ? 1 : 0, c->bf16 ? vec.p : nullptr));
  if (!c->dry && c->taps && c->taps->style_vec)
    HIPCHK(c, hipMemcpyAsync(c->taps->style_vec, c->bf16 ? vec32.p : vec.p, (size_t)B * 96 * 4, hipMemcpyDeviceToDevice, c->st));
  P.free(xs);
  P.free(part);
  if (!c->bf16) P.free(vec32);        // bf16 mode: the fp32 vector feeds the bias table of conv11 (released after the decoder)
  if (P.side_end()) return 1;
  // ---- coarse branch :138-147
  Act xc = encoder(P, "conv", cin, nullptr);
  if (P.rc) return P.rc;
  if (P.join()) return 1;
  float* vb = P.alloc_raw((size_t)B * 9 * 192);     // bias table of the folded style vector (run_gconv)
  if (P.rc) return P.rc;
  c->vbias_ws = vb;
  c->vec32 = c->bf16 ? vec32.p : nullptr;
  Act d = decoder(P, "conv", xc, vec.p, 96, 1);     // :167-175 (cat is virtual)
  c->vbias_ws = nullptr; c->vec32 = nullptr;
  P.release(vb);
  if (c->bf16) P.free(vec32);
  P.free(vec);
  Act xnow = P.alloc(H, W, 4);
  if (P.rc) return P.rc;
  small(P, "conv17", d, 2, coarse_out, nullptr, x, mask, xnow.p, nullptr, (flags & SE_FLAG_NO_MASK_COARSE) ? 1 : 0);
  if (P.rc) return P.rc;
  // ---- patch-match branch :197-209 (side)
  if (P.side_begin()) return 1;
  Act pm = P.conv("pmconv1", xnow, false);
  pm = P.conv("pmconv2_downsample", pm);
  pm = P.conv("pmconv3", pm);
  pm = P.conv("pmconv4_downsample", pm);
  pm = P.conv("pmconv5", pm);
  pm = P.conv("pmconv6", pm);
  if (P.rc) return P.rc;
  if (!c->dry && c->taps && c->taps->pmconv6)
    HIPCHK(c, (c->bf16 ? launch_nhwc16_to_nchw : launch_nhwc_to_nchw)(pm.p, c->taps->pmconv6, B, 96, 96, pm.H, pm.W, c->st));
  if (flags & SE_FLAG_USE_CAM) {
    Act att = P.alloc(pm.H, pm.W, 96);
    if (P.rc) return P.rc;
    if (run_attention(c, P, pm, mask, att, nullptr)) return P.rc ? P.rc : 1;
    P.free(pm);
    pm = att;
    if (!c->dry && c->taps && c->taps->attn_out)
      HIPCHK(c, (c->bf16 ? launch_nhwc16_to_nchw : launch_nhwc_to_nchw)(pm.p, c->taps->attn_out, B, 96, 96, pm.H, pm.W, c->st));
  }
  pm = P.conv("pmconv9", pm);
  pm = P.conv("pmconv10", pm);
  if (P.rc) return P.rc;
  if (P.side_end()) return 1;
  // ---- hallucination branch :184-194
  Act hcur = P.conv("xconv1", xnow, false);
  hcur = P.conv("xconv2_downsample", hcur);
  hcur = P.conv("xconv3", hcur);
  hcur = P.conv("xconv4_downsample", hcur);
  hcur = P.conv("xconv5", hcur);
  hcur = P.conv("xconv6", hcur);
  hcur = P.conv("xconv7_atrous", hcur);
  hcur = P.conv("xconv8_atrous", hcur);
  hcur = P.conv("xconv9_atrous", hcur);
  Act hallu = P.conv("xconv10_atrous", hcur);
  if (P.rc) return P.rc;
  if (P.join()) return 1;
  P.free(xnow);                                         // read by both branches: released after the join
  Act d2 = decoder(P, "allconv", hallu, pm.p, 96, 0);   // cat([x_hallu, pm]) :211 is virtual
  P.free(pm);
  small(P, "allconv17", d2, 3, fine_out, nullptr, x, soft_mask, nullptr, soft_mask ? composed_out : nullptr, 0, packed_bs, nullptr,
        (flags & SE_FLAG_RAW_FINE) != 0);
  c->rgb8 = nullptr; c->m8 = nullptr;
  return P.rc;
}

// Row stride (in elements) of the R x R matrices E, P, P~ and of the transposed values: R rounded up to whole k-chunks
// (32 fp32 / 64 bf16 keys).  (Padding the power-of-two strides of 256x256 / 512x512 inputs by one chunk was measured:
// no gain for the row-streaming passes -- they are not camping on HBM channels.)
int att_row_stride(int R, bool bf) {
  const int chunk = bf ? 64 : 32;
  int Rp = (R + chunk - 1) / chunk * chunk;
  return Rp;
}

// Whether attention on an h x w feature map runs in the streaming form (se_att_stream.hip: nothing R x R): wherever the
// materialised space-to-depth form cannot address its R x R matrices with 32-bit offsets (R Rp 4 >= 2^31), and everywhere
// with SE_ATT_STREAM=1 unless `similar_out` -- P itself -- is asked for.  `similar_out` is refused exactly where
// R Rp 4 >= 2^31, whatever the options (Engine.attention checks the same rule before it allocates the L x L output).
bool att_streaming(int h, int w, bool bf, bool want_similar) {
  const int R = (h / 2) * (w / 2), Rp = att_row_stride(R, bf);
  const bool fits = (double)R * Rp * 4.0 < 2147483648.0;
  if (want_similar && !fits) return true;              // (run_attention refuses: similar_out is P itself)
  if (opt(OPT_ATT_STREAM) == 1 && !want_similar) return true;
  return !fits;
}

int run_attention(se_ctx* c, Plan& P, Act& x, const float* mask_full, Act& out, float* similar_nchw) {
  const int h = x.H, w = x.W, B = P.B;
  const int hs = (h - 4) / 2 + 1, ws = (w - 4) / 2 + 1, L = hs * ws, Lp = (L + 31) & ~31;
  const bool bf = c->bf16;
  const bool stream = att_streaming(h, w, bf, similar_nchw != nullptr);
  const int hc = h / 2, wc = w / 2, R = hc * wc;
  const int Rp = att_row_stride(R, bf);
  const int guard = (wc + 8 + 63) & ~63;               // floats; att2_ptilde_kernel reads up to wc + 5 columns outside a row
  if (stream && similar_nchw)
    return P.rc = fail(c, "attention: similar_out (the %d x %d score matrix) is not available on a %dx%d feature map: "
                          "it runs in the streaming form, which never forms it", L, L, h, w);
  // fp32 scratch is sized in floats whatever the activation type
  float* part = P.alloc_raw((size_t)B * COLREDUCE_SPLITS * 96);
  float* rn = P.alloc_raw((size_t)B * 96);
  float* xn = P.alloc_raw(bf ? ((size_t)B * h * w * 96 + 1) / 2 : (size_t)B * h * w * 96);
  float *valid = nullptr, *S = nullptr, *S2 = nullptr, *xT = nullptr, *stats = nullptr;
  if (stream) {      // O(R): validR, kmul, kadd; (max, 1 / sum) per query; V^T plus the tail the out pass may read
    valid = P.alloc_raw(3 * (size_t)B * Rp);
    stats = P.alloc_raw((size_t)B * R * 2);
    xT = P.alloc_raw((bf ? (size_t)B * 4 * 96 * Rp / 2 : (size_t)B * 4 * 96 * Rp) + att_stream_xt_tail());
  } else {
    valid = P.alloc_raw(7 * ((size_t)B * Rp + guard) + (size_t)B * 768 + (size_t)B * hc * 384);      // validR, kmul, kadd (+ fp16-E form: kadd2, ea4, ea, eb), each behind its guard band; emean, epart
    stats = P.alloc_raw((size_t)B * R * 2);    // fused streaming pass: (row max, 1 / row sum) per query
    xT = P.alloc_raw(bf ? (size_t)B * 4 * 96 * Rp / 2 : (size_t)B * 4 * 96 * Rp);
    S = P.alloc_raw((size_t)B * R * Rp + 2 * guard);       // E (fp32) between two guard bands; three-pass form: then P~
    S2 = P.alloc_raw(bf ? (size_t)B * R * Rp / 2 : (size_t)B * R * Rp);      // P (fp32 / bf16)
  }
  if (P.rc) return P.rc;
  if (!c->dry) {
    HIPCHK(c, launch_colreduce(x.p, part, rn, B, h * w, 96, 2, c->st, bf ? 1 : 0));
    AttParams a;
    memset(&a, 0, sizeof a);
    a.x = x.p; a.rn = rn; a.xn = xn; a.hard = mask_full; a.out = out.p;
    a.B = B; a.h = h; a.w = w; a.hs = hs; a.ws = ws; a.L = L; a.Lp = Lp;
    a.scale = 10.f; a.th = 0.1f;                        // editline_g.py:35-38
    if (stream) {
      a.hc = hc; a.wc = wc; a.R = R; a.Rp = Rp; a.bf16 = bf ? 1 : 0;
      a.validR = valid; a.kmul = valid + (size_t)B * Rp; a.kadd = valid + 2 * (size_t)B * Rp;
      a.xT = xT; a.stats = stats;
      HIPCHK(c, launch_attention_stream(a, c->st));
    } else {
      a.hc = hc; a.wc = wc; a.R = R; a.Rp = Rp; a.bf16 = bf ? 1 : 0;
      a.validR = valid + guard; a.xT = xT; a.E = S + guard; a.P = S2; a.stats = stats; a.guard = guard; a.similar = similar_nchw;
      a.kmul = valid + ((size_t)B * Rp + guard) + guard; a.kadd = valid + 2 * ((size_t)B * Rp + guard) + guard;
      a.kadd2 = valid + 3 * ((size_t)B * Rp + guard) + guard; a.ea4 = valid + 4 * ((size_t)B * Rp + guard) + guard;
      a.ea = valid + 5 * ((size_t)B * Rp + guard) + guard; a.eb = valid + 6 * ((size_t)B * Rp + guard) + guard;
      a.emean = valid + 7 * ((size_t)B * Rp + guard); a.epart = a.emean + (size_t)B * 768;
      HIPCHK(c, launch_attention(a, c->st));
    }
  }
  P.release(S2); P.release(S); P.release(xT); P.release(stats); P.release(valid);
  P.release(xn); P.release(rn); P.release(part);
  return 0;
}

}  // namespace se

namespace {

// Passes of a forward over a large batch.  The kernels address a tensor with 32-bit byte offsets (addr_limit); the largest
// tensor of either network is the 24-channel full-resolution activation (conv1 / conv15_upsample outputs: 96 bytes per
// pixel in fp32, 48 in bf16 -- max_act_bytes_per_image derives it from the plans), so a forward runs over at most
// (limit - 1) / (H W 96) images at a time and a larger batch is
// run as several passes of the SAME plan over image ranges -- same kernels, same execution mode, so an image's result does
// not depend on the pass it lands in (bit for bit: test_large_batch_is_split_into_passes).  Passes are balanced
// (ceil(B / passes) images each).  Returns the images per pass, or 0 (error set) when ONE image exceeds the range.
// bytes per image of the LARGEST activation tensor either plan allocates at this size -- derived from a dry run of the plans
// themselves (the literal "24 channels at full resolution = 96 / 48 bytes per pixel" would silently go stale with
// a wider layer); cached per (H, W, precision)
long long max_act_bytes_per_image(se_ctx* c, int H, int W, int flags) {
  const std::vector<long long> key = {H, W, (flags & SE_FLAG_BF16) ? 1 : 0};
  auto it = c->act_per_img.find(key);
  if (it != c->act_per_img.end()) return it->second;
  const bool dry0 = c->dry, ll0 = c->low_latency, bf0 = c->bf16, pair0 = c->paired;
  c->dry = true; c->low_latency = false; c->bf16 = (flags & SE_FLAG_BF16) != 0; c->paired = false;
  c->dry_max_act = 0;
  float dummy;
  c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
  plan_netM(c, nullptr, nullptr, nullptr, nullptr, &dummy, 1, H, W, 0);
  c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
  plan_netG(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, H, W, SE_FLAG_USE_CAM | SE_FLAG_POOL_MAX, 0);
  c->dry = dry0; c->low_latency = ll0; c->bf16 = bf0; c->paired = pair0;
  const long long v = (long long)c->dry_max_act;
  c->act_per_img[key] = v;
  return v;
}

}  // namespace

namespace se {

int pass_size(se_ctx* c, int B, int H, int W, int flags) {
  const long long per_img = max_act_bytes_per_image(c, H, W, flags);
  const long long lim = addr_limit();
  if (per_img <= 0) { fail(c, "internal: no activation size for %dx%d", H, W); return 0; }
  if (per_img >= lim) {
    fail(c, "a %dx%d image exceeds the kernels' 32-bit byte offsets (%lld bytes per activation, limit %lld)", H, W, per_img, lim);
    return 0;
  }
  const long long bmax = (lim - 1) / per_img;
  if (B <= bmax) return B;
  const long long passes = (B + bmax - 1) / bmax;
  return (int)((B + passes - 1) / passes);
}

// Arena peaks of a forward, from a dry run of the very plan that will be launched (nothing is enqueued): main-branch
// arena and, in low-latency mode, the side-branch arena.  which: 1 netM, 2 netG, 3 netM then netG (se_inference).
// pair (pair_pass): the B images run as two halves, each planned as the enqueue loop plans it -- the first half's chain in the
// main arena, the second's in the side arena; the peaks are those of the two chains.
se_ctx::Peaks plan_peaks(se_ctx* c, int which, int B, int H, int W, int flags, bool want_maskim, bool pair) {
  const std::vector<long long> key = {which, B, H, W,
                                      flags & (SE_FLAG_USE_CAM | SE_FLAG_JOINT_TRAIN_INP | SE_FLAG_LOW_LATENCY | SE_FLAG_BF16),
                                      want_maskim ? 1 : 0, c->fork2 ? 1 : 0, opt_epoch(), c->serial ? 1 : 0, pair ? 1 : 0};
  auto it = c->peaks.find(key);
  if (it != c->peaks.end()) return it->second;
  const bool dry0 = c->dry, ll0 = c->low_latency, bf0 = c->bf16, pair0 = c->paired;
  const int half0 = c->half;
  c->dry = true;
  c->low_latency = (flags & SE_FLAG_LOW_LATENCY) != 0;
  c->bf16 = (flags & SE_FLAG_BF16) != 0;
  float dummy;      // non-null marker for optional outputs
  se_ctx::Peaks pk{0, 0};
  for (int half = 0; half < (pair ? 2 : 1); ++half) {
    const int nb = !pair ? B : half ? B - pair_first(B) : pair_first(B);
    c->paired = pair; c->half = half;
    if (which & 1) {
      c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
      plan_netM(c, nullptr, nullptr, nullptr, nullptr, want_maskim ? &dummy : nullptr, nb, H, W);
      if (c->arena.peak > pk.main) pk.main = c->arena.peak;
      if (c->arena2.peak > pk.side) pk.side = c->arena2.peak;
    }
    if (which & 2) {
      c->arena.reset(nullptr, 0, true, 0); c->arena2.reset(nullptr, 0, true, 1);
      plan_netG(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nb, H, W, flags);
      if (c->arena.peak > pk.main) pk.main = c->arena.peak;
      if (c->arena2.peak > pk.side) pk.side = c->arena2.peak;
    }
  }
  c->dry = dry0; c->low_latency = ll0; c->bf16 = bf0; c->paired = pair0; c->half = half0;
  c->peaks[key] = pk;
  return pk;
}

// One fork in front of both halves of a paired pass and one join behind them, with the ctx's own events: the side stream starts
// behind everything the caller's stream holds so far (the previous pass and call with it), the caller's stream goes on behind both halves.
int pair_fork(se_ctx* c, hipStream_t main) {
  HIPCHK(c, hipEventRecord(c->ev_fork, main));
  HIPCHK(c, hipStreamWaitEvent(c->st_side, c->ev_fork, 0));
  return 0;
}
// after begin_call: the plans that follow are half `half` of a paired pass (Plan::home, Plan::forked)
void pair_half(se_ctx* c, int half) {
  c->paired = true; c->half = half;
  c->st = half ? c->st_side : c->st_main;
}
int pair_join(se_ctx* c, hipStream_t main) {
  c->paired = false; c->half = 0; c->st = main;
  HIPCHK(c, hipEventRecord(c->ev_join, c->st_side));
  HIPCHK(c, hipStreamWaitEvent(main, c->ev_join, 0));
  return 0;
}

// carve the caller's workspace into the arenas of this call; `tail` bytes at the end stay reserved.  (A paired pass: pk holds
// the two halves' peaks, the same two regions serve them.)
int carve(se_ctx* c, const se_ctx::Peaks& pk, void* ws, size_t ws_bytes, size_t tail) {
  if (ws_bytes < pk.main + pk.side + tail)
    return fail(c, "workspace too small: %zu bytes, this call needs %zu", ws_bytes, pk.main + pk.side + tail);
  // the main arena gets whatever the side arena does not need
  c->arena.reset((char*)ws, ws_bytes - tail - pk.side, false);
  c->arena2.reset((char*)ws + (ws_bytes - tail - pk.side), pk.side, false);
  return 0;
}

}  // namespace se
