"""References, an fp32 emulation, elementwise checkers and the case list for sf_conv_igemm (csrc/conv_igemm.hip and
csrc/conv_halo.hip) and for the channel RMS-norm + SiLU, fused (the halo kernel's norm_out) or not (sf_rmsnorm_silu_cl).
Host-only, plain torch; tests/test_conv_kernels_host.py runs it on the CPU, tests/test_gpu_conv_kernels.py holds the
kernels to it.

Layers, all on the same bf16 inputs:

  conv_reference   float64, the statement above sf_conv_args in include/sf_hip.h taken literally: a loop over the taps,
                   zero padding, `upsample`, `t_in_offset`, `stride_hw` / `stride_t`, bias, residual, the channel -> frame
                   interleave and the clamped planar float head.  The result is indexed like the kernel's output BUFFER
                   (frames in front of `out_frame_offset` and one frame behind the volume, `ldo` channels per row), with the
                   mask of the elements a launch owns.  `absacc` is the same sum over |x| |w| (taps only).
  norm_reference   float64 RMS_norm (+ SiLU) of the kernel's OWN bf16 raw row.
  fp32_emulation   what a correct fp32 implementation gives: the taps accumulated in fp32, bias and residual added in fp32,
                   ONE rounding to bf16 (the raw output), the norm evaluated in fp32 on the rounded values with
                   x * rcp(1 + exp2(-log2(e) x)) for SiLU, one more rounding.  It is not the code under test; it shows that
                   the checkers accept a correct implementation, and, with `bug=`, that they reject ten wrong ones.
  check_*          compare a buffer with a reference at EVERY owned element and raise Mismatch with the first bad index as
                   (t, h, w, n) (buffer coordinates; the planar float head: (t, n, h, w)), the number of bad elements and the
                   worst err / tol.
  Canary           an output buffer between two guard bands, pre-filled with a NaN bit pattern; after a launch everything
                   the launch does not own must still hold that pattern.

Data families (make_data):

  "int"    x integers in [-4, 4], w in [-2, 2], bias and residual integers in [-8, 8]: all exact in bf16.  Every product
           and every partial sum is an integer below K * 8 + 16 <= 3456 * 8 + 16 < 2^24, hence exact in fp32 in ANY order
           of summation, on any matrix unit.  The kernel's fp32 value is therefore the exact value, and its bf16 output must
           equal ONE round-to-nearest-even of it bit for bit (round_once_to_bf16: integer arithmetic on the float64 bits).
           The float head's w and bias are scaled by the power of two that puts closest to 5 % of the results beyond +-1
           (still exact; a factor of two moves that share a long way: 17 % at the head case's K = 2592, the next power
           leaves 0.5 %): the float output is then exactly the clamped reference.
  "gauss"  x ~ N(0, 1), w ~ N(0, 1 / K), bias ~ N(0, 0.1^2), residual ~ N(0, 1): the scales of tests/test_gpu_vae.py.
           Bound, as tests/test_gpu_gemm_batched.py derives it, K = taps * Cin:
               bf16 output   |out - ref| <= 2^-8 |ref| + K 2^-22 absacc
               fp32 head     |out - ref| <= K 2^-22 absacc + 2^-23 |ref|     (the clamp is 1-Lipschitz: the bound of the
                                                                              unclamped value carries through it)
           2^-8 |ref| is the one rounding to bf16; (K - 1) 2^-24 absacc bounds an fp32 accumulation of exact bf16 products
           in any order, x 4 because the MFMA's internal rounding mode is not documented; 2^-23 |ref| is the fp32 bias add.
           With Cin > 128 the accumulation term dominates and the bound loses its teeth: the Gaussian cases keep
           Cin <= 128, and the integer family covers the rest.

Dispatch (dispatch): which kernel a launch reaches, mirrored from sf_conv_igemm / sf_conv_halo_launch / sf_conv_pick_nt:
the halo domain, the 160-tile rule between the halo kernel's two widths, the column tile of the implicit GEMM, its two
epilogues and the parity of the slice count.  The host test asserts that CASES reaches every one of them."""
import dataclasses
import functools
import math
import zlib

import torch

BF16 = torch.bfloat16
GUARD = 512                                    # elements in front of and behind every canary buffer (keeps 16-byte alignment)
FILL = {torch.bfloat16: 0x7FA5, torch.float32: 0x7FC5A5A5}     # quiet NaNs with a payload
INT = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
LOG2E_F32 = 1.44269504088896                   # the constant of silu_fast_f (csrc/sf_common.h)


# ------------------------------------------------------------------------------------------ cases
@dataclasses.dataclass(frozen=True)
class ConvCase:
    """One launch of sf_conv_igemm.  (Hin, Win) is the INPUT frame; the output frame follows from upsample / stride_hw."""
    name: str
    Cin: int
    Cout: int
    kt: int
    ks: int                      # spatial taps per side: 3 or 1
    T: int                       # output frames (before the interleave doubles them)
    Hin: int
    Win: int
    upsample: bool = False
    stride_hw: int = 1
    stride_t: int = 1
    t_in_offset: int = 0
    epilogue: str = "bias"       # "bias", "resid", "clamp"
    ldo: int = 0                 # 0: tight
    ldr: int = 0                 # 0: as ldo
    out_frame_offset: int = 0
    interleave: bool = False
    norm: bool = False
    norm_ld: int = 0             # 0: tight
    norm_frame_offset: int = 0
    out_null: bool = False       # norm only
    resid_alias: bool = False    # resid is the output buffer itself
    ldw_extra: int = 0           # weight columns behind roundup(K, 64): NaN
    structure: str = "igemm"     # what the launch forces: "igemm", "halo", or "auto"
    family: str = "int"

    @property
    def H(self):
        return 2 * self.Hin if self.upsample else self.Hin // 2 if self.stride_hw == 2 else self.Hin

    @property
    def W(self):
        return 2 * self.Win if self.upsample else self.Win // 2 if self.stride_hw == 2 else self.Win

    @property
    def taps(self):
        return self.kt * self.ks * self.ks

    @property
    def K(self):
        return self.taps * self.Cin

    @property
    def kpad(self):
        return (self.K + 63) // 64 * 64

    @property
    def ldw(self):
        return self.kpad + self.ldw_extra

    @property
    def out_channels(self):
        return self.Cout // 2 if self.interleave else self.Cout

    @property
    def out_frames(self):
        return 2 * self.T if self.interleave else self.T

    @property
    def ldo_(self):
        return self.ldo or self.out_channels

    @property
    def ldr_(self):
        return self.ldo_ if self.resid_alias else (self.ldr or self.ldo_)

    @property
    def norm_ld_(self):
        return self.norm_ld or self.Cout

    @property
    def x_frames_used(self):     # frames [t_in_offset, this) are all the launch may read
        return self.t_in_offset + self.stride_t * (self.T - 1) + self.kt

    @property
    def out_shape(self):         # the output BUFFER: one unowned frame behind the volume
        if self.epilogue == "clamp":
            return (self.T + 1, self.Cout, self.H, self.W)
        return (self.out_frame_offset + self.out_frames + 1, self.H, self.W, self.ldo_)

    @property
    def norm_shape(self):
        return (self.norm_frame_offset + self.T + 1, self.H, self.W, self.norm_ld_)

    def data_key(self):
        """Launches of one convolution in different forms (structure, ldo, norm, frame offsets) share their tensors."""
        return (self.Cin, self.Cout, self.kt, self.ks, self.Hin, self.Win, self.upsample, self.epilogue == "clamp", self.family)


def pick_nt(cout):
    """sf_conv_pick_nt: the column tile (32 NT) that pads Cout least; ties go to the larger tile."""
    best, best_cost = 1, None
    for nt in (6, 4, 3, 2, 1):
        cost = (cout + 32 * nt - 1) // (32 * nt) * 32 * nt
        if best_cost is None or cost < best_cost:
            best, best_cost = nt, cost
    return best


def halo_takes(c):
    """The domain of sf_conv_halo_launch."""
    if c.stride_hw > 1 or c.stride_t > 1 or c.ks != 3 or c.interleave or c.Cin % 32 or c.H < 16 or c.W < 16:
        return False
    if c.epilogue == "clamp":
        return c.Cout <= 4 and not c.norm
    if c.Cout % 8 or (not c.out_null and c.ldo_ % 8):
        return False
    if c.norm and not (c.Cout in (96, 192) and c.norm_ld_ >= c.Cout and c.norm_ld_ % 8 == 0):
        return False
    if c.out_null and not c.norm:
        return False
    return c.Cout % 96 == 0


def dispatch(c, structure=None):
    """The kernel a launch reaches: ("halo", NT, tiles_n), ("halo_head",), ("igemm", NT, "lds" | "direct", "odd" | "even")
    or ("refused",)."""
    s = structure or c.structure
    if s != "igemm" and halo_takes(c):
        if c.epilogue == "clamp":
            return ("halo_head",)
        nt = 6 if c.Cout % 192 == 0 else 3
        patches = c.T * ((c.H + 15) // 16) * ((c.W + 15) // 16)
        if nt == 6 and not c.norm and patches * (c.Cout // 192) < 160:
            nt = 3
        return ("halo", nt, c.Cout // (32 * nt))
    if s == "halo" or c.norm or (c.out_null and c.epilogue != "clamp"):
        return ("refused",)
    direct = c.epilogue == "clamp" or c.interleave or c.Cout % 8 != 0 or c.ldo_ % 8 != 0
    return ("igemm", pick_nt(c.Cout), "direct" if direct else "lds", "odd" if (c.taps * (c.Cin // 32)) % 2 else "even")


def _cases():
    R = dataclasses.replace
    halo = [
        # one ragged patch row and column, the output inside a wider buffer behind one foreign frame
        ConvCase("halo96_ragged", 32, 96, 3, 3, 2, 17, 33, t_in_offset=1, ldo=104, out_frame_offset=1, ldw_extra=64, structure="halo"),
        # nine planes (3 slices x 3 frames): the ring of four plane slots wraps
        ConvCase("halo96_ring_resid", 96, 96, 3, 3, 1, 31, 16, epilogue="resid", ldr=112, structure="halo"),
        # (as the decoder's conv2 runs: x += conv2(...) in place, and the next block's normalised input beside it)
        ConvCase("halo96_ring_alias", 96, 96, 3, 3, 1, 31, 16, epilogue="resid", resid_alias=True, norm=True, ldw_extra=128, structure="halo"),
        ConvCase("halo96_ring_norm", 96, 96, 3, 3, 1, 31, 16, norm=True, norm_ld=128, norm_frame_offset=2, structure="halo"),
        # the 192-column tile at a small shape, three ways
        ConvCase("halo192_both", 64, 192, 3, 3, 2, 20, 23, t_in_offset=1, norm=True, ldw_extra=64, structure="halo"),
        ConvCase("halo192_norm_only", 64, 192, 3, 3, 2, 20, 23, t_in_offset=1, norm=True, out_null=True, ldw_extra=64, structure="halo"),
        ConvCase("halo192_out_only", 64, 192, 3, 3, 2, 20, 23, t_in_offset=1, ldw_extra=64, structure="halo"),
        # 2 x 7 x 6 patches x 2 column tiles = 168 tiles: the wide tile without a norm
        ConvCase("halo384_two_column_tiles", 32, 384, 1, 3, 2, 100, 90, ldw_extra=64, structure="halo"),
        ConvCase("halo_up96", 128, 96, 1, 3, 2, 9, 13, upsample=True, norm=True, structure="halo"),
        ConvCase("halo_up192", 128, 192, 1, 3, 2, 9, 13, upsample=True, norm=True, norm_ld=200, ldw_extra=64, structure="halo"),
        # every halo edge out of range
        ConvCase("halo_border_16x16", 32, 96, 3, 3, 1, 16, 16, ldw_extra=64, structure="halo"),
        ConvCase("halo_border_48x16", 32, 192, 1, 3, 1, 48, 16, norm=True, structure="halo"),
        ConvCase("halo_head", 96, 3, 3, 3, 2, 19, 37, t_in_offset=1, epilogue="clamp", ldw_extra=64, structure="halo"),
    ]
    halo += [R(c, name=c.name + "_gauss", family="gauss") for c in halo if c.name in ("halo96_ragged", "halo192_both", "halo_head")]
    ig = []
    for c in halo:   # the same launches through the implicit GEMM, which has no norm output
        twin = R(c, name="ig_" + c.name.replace("_both", ""), structure="igemm", norm=False, norm_ld=0, norm_frame_offset=0, out_null=False)
        if all(dataclasses.replace(twin, name="") != dataclasses.replace(o, name="") for o in ig):
            ig.append(twin)
    for cout in (32, 64, 96, 128, 192, 160, 40, 100):       # NT 1, 2, 3, 4, 6; five column tiles; ragged column tiles
        ig.append(ConvCase(f"ig_cout{cout}", 32, cout, 3, 3, 3, 5, 9, ldw_extra=64 if cout in (64, 128, 160, 100) else 0))
    ig += [
        ConvCase("ig_cout100_gauss", 32, 100, 3, 3, 3, 5, 9, ldw_extra=64, family="gauss"),
        ConvCase("ig_even_slices", 64, 96, 3, 3, 2, 5, 7, t_in_offset=1),
        # the direct epilogue's Cout % 8 == 4 and ldo % 8 == 4 entries; M = 105: a ragged row tile
        ConvCase("ig_cout36_ldo36", 32, 36, 3, 3, 3, 5, 7, epilogue="resid", ldo=36, ldr=40),
        ConvCase("ig_cout36_ldo44", 32, 36, 3, 3, 3, 5, 7, epilogue="resid", ldo=44, ldr=40, ldw_extra=64),
        ConvCase("ig_1x1_m1", 32, 64, 1, 1, 1, 1, 1, ldw_extra=64),
        ConvCase("ig_1x1_m129", 64, 32, 1, 1, 1, 3, 43),
        ConvCase("ig_interleave", 32, 128, 3, 1, 2, 5, 7, ldo=72, out_frame_offset=2, interleave=True, ldw_extra=64),
        # odd input: the right / bottom taps of the last output row and column read zero, the last input row is unused
        ConvCase("ig_stride_hw", 32, 64, 1, 3, 2, 11, 13, stride_hw=2),
        ConvCase("ig_stride_t", 64, 64, 3, 1, 2, 5, 7, stride_t=2, t_in_offset=1, ldw_extra=64),
        # ldo % 8 == 4 is outside the halo domain: AUTO falls back to the implicit GEMM's direct epilogue
        ConvCase("auto_ldo100_falls_back", 32, 96, 3, 3, 1, 17, 16, ldo=100, structure="auto"),
    ]
    return halo, ig


HALO_CASES, IGEMM_CASES = _cases()
CASES = HALO_CASES + IGEMM_CASES
REQUIRED_DISPATCH = ([("halo", 3, 1), ("halo", 6, 1), ("halo", 6, 2), ("halo_head",)]
                     + [("igemm", nt) for nt in (1, 2, 3, 4, 6)] + ["lds", "direct", "odd", "even"])


def dispatch_table(cases=None):
    return {c.name: dispatch(c) for c in (cases or CASES)}


def dispatch_coverage(cases=None):
    """The items of REQUIRED_DISPATCH that the case list reaches."""
    got = set()
    for d in dispatch_table(cases).values():
        if d[0] == "igemm":
            got |= {("igemm", d[1]), d[2], d[3]}
        else:
            got.add(d)
    return got


# ------------------------------------------------------------------------------------------ data
@dataclasses.dataclass
class ConvData:
    x: torch.Tensor              # bf16 [frames][Hin][Win][Cin]; frames the launch must not read hold NaN
    w: torch.Tensor              # bf16 [Cout][ldw]; columns [K, kpad) zero, [kpad, ldw) NaN
    bias: torch.Tensor           # bf16 [Cout]
    resid: torch.Tensor          # bf16, one row of channels per output position of every frame of the output buffer
    gamma: torch.Tensor          # bf16 [Cout], within 1 +- 0.5


def _seed(c):
    return zlib.crc32(repr(c.data_key()).encode())


DATA_FRAMES = 8                                # input frames generated per convolution; a case reads a prefix of them


@functools.lru_cache(maxsize=8)
def _base_data(key, seed):
    """x [DATA_FRAMES][Hin][Win][Cin], taps [Cout][K], bias, gamma of one convolution (no NaN yet)."""
    T_frames = DATA_FRAMES
    cin, cout, kt, ks, hin, win, _, head, family = key
    K = kt * ks * ks * cin
    g = torch.Generator().manual_seed(seed)
    if family == "int":
        x = torch.randint(-4, 5, (T_frames, hin, win, cin), generator=g).to(BF16)
        w = torch.randint(-2, 3, (cout, K), generator=g).to(BF16)
        bias = torch.randint(-8, 9, (cout,), generator=g).to(BF16)
    else:
        x = torch.randn((T_frames, hin, win, cin), generator=g).to(BF16)
        w = (torch.randn((cout, K), generator=g) * K ** -0.5).to(BF16)
        bias = (torch.randn((cout,), generator=g) * 0.1).to(BF16)
    gamma = (1 + 0.25 * torch.randn((cout,), generator=g)).clamp(0.5, 1.5).to(BF16)
    return x, w, bias, gamma


def make_data(c):
    """The tensors of a case, seeded by the convolution alone (data_key): launches that differ in T, t_in_offset or the
    output's form see the same frames.  Frames in front of t_in_offset and one frame behind the last tap hold NaN."""
    used = c.x_frames_used
    assert used <= DATA_FRAMES
    x, w, bias, gamma = _base_data(c.data_key(), _seed(c))
    x = torch.cat([x[:used], torch.full((1,) + tuple(x.shape[1:]), float("nan"), dtype=BF16)]).clone()
    x[:c.t_in_offset] = float("nan")
    if c.epilogue == "clamp" and c.family == "int":
        # the power of two that puts closest to 5 % (as a ratio) of the results beyond +-1; w and bias stay exact in bf16
        y = _accumulate(c, x, w, torch.float64) + bias.double()
        shift = min(range(0, 16), key=lambda s: abs(math.log(max(float((y.abs() > 2.0 ** s).double().mean()), 1e-9) / 0.05)))
        w, bias = (w.double() * 2.0 ** -shift).to(BF16), (bias.double() * 2.0 ** -shift).to(BF16)
    wp = torch.full((c.Cout, c.ldw), float("nan"), dtype=BF16)
    wp[:, :c.kpad] = 0
    wp[:, :c.K] = w
    resid = None
    if c.epilogue == "resid":
        g = torch.Generator().manual_seed(_seed(c) + 1)
        F, H, W, _ = c.out_shape
        full = (torch.randint(-8, 9, (F, H, W, c.Cout), generator=g) if c.family == "int" else torch.randn((F, H, W, c.Cout), generator=g)).to(BF16)
        resid = torch.zeros((F, H, W, c.ldr_), dtype=BF16)      # every frame holds values: a read of the wrong frame is a wrong number
        resid[..., :c.Cout] = full
    return ConvData(x, wp, bias, resid, gamma)


# ------------------------------------------------------------------------------------------ the convolution itself
def _tap_index(c, pos, d, n_in, n_out, bug):
    """Input coordinate and validity of tap d (0 .. ks - 1) for the output coordinates `pos` along one spatial axis."""
    if c.stride_hw == 2:
        v = 2 * pos + d - (1 if bug == "stride_pad_left" else 0)
        return v.clamp(0, n_in - 1), (v >= 0) & (v < n_in)
    v = pos + d - c.ks // 2
    ok = (v >= 0) & (v < (n_out if c.upsample else n_in))
    if c.upsample:
        v = (v + 1) >> 1 if bug == "upsample_round_up" else v >> 1
    return v.clamp(0, n_in - 1), ok


def _accumulate(c, x, w, dtype, bug=None):
    """sum over taps and input channels, [T][H][W][Cout] in `dtype`, one matrix product per tap."""
    T, H, W = c.T, c.H, c.W
    t, h, wv = torch.arange(T), torch.arange(H), torch.arange(W)
    y = torch.zeros((T * H * W, c.Cout), dtype=dtype)
    for dt in range(c.kt):
        frames = x[c.stride_t * t + dt + c.t_in_offset].to(dtype)
        for dh in range(c.ks):
            hi, hm = _tap_index(c, h, dh, c.Hin, H, bug)
            for dw in range(c.ks):
                wi, wm = _tap_index(c, wv, dw, c.Win, W, bug)
                m = (hm[:, None] & wm[None, :]).clone()
                if bug == "drop_corner_tap" and (dt, dh, dw) == (0, 0, 0):
                    m[H - 1, W - 1] = False          # a valid tap of the last pixel treated as padding
                xs = frames[:, hi][:, :, wi] * m[None, :, :, None].to(dtype)
                tap = (dt * c.ks + dh) * c.ks + dw
                y += xs.reshape(T * H * W, c.Cin) @ w[:, tap * c.Cin:(tap + 1) * c.Cin].to(dtype).T
    return y.view(T, H, W, c.Cout)


def _to_buffer(c, y, fill):
    """[T][H][W][Cout] -> the output buffer's indexing; unowned elements hold `fill`."""
    if c.epilogue == "clamp":
        buf = torch.full(c.out_shape, fill, dtype=y.dtype)
        buf[:c.T] = y.permute(0, 3, 1, 2)
        return buf
    if c.interleave:
        ic = c.Cout // 2
        y = y.view(c.T, c.H, c.W, 2, ic).permute(0, 3, 1, 2, 4).reshape(2 * c.T, c.H, c.W, ic)
    buf = torch.full(c.out_shape, fill, dtype=y.dtype)
    buf[c.out_frame_offset:c.out_frame_offset + c.out_frames, :, :, :c.out_channels] = y
    return buf


def owned_mask(c):
    return _to_buffer(c, torch.ones((c.T, c.H, c.W, c.Cout), dtype=torch.bool), False)


def norm_owned_mask(c):
    m = torch.zeros(c.norm_shape, dtype=torch.bool)
    m[c.norm_frame_offset:c.norm_frame_offset + c.T, :, :, :c.Cout] = True
    return m


def _resid_rows(c, d, dtype, bug=None):
    f0 = c.out_frame_offset + (1 if bug == "resid_next_frame" else 0)
    return d.resid[f0:f0 + c.T, :, :, :c.Cout].to(dtype)


@dataclasses.dataclass
class ConvRef:
    ref: torch.Tensor            # float64, the output buffer's shape; NaN where the launch owns nothing
    absacc: torch.Tensor         # float64, same indexing (None if not asked for)
    owned: torch.Tensor          # bool


def conv_reference(c, d, absacc=True):
    y = _accumulate(c, d.x, d.w, torch.float64) + d.bias.double()
    if c.epilogue == "resid":
        y = y + _resid_rows(c, d, torch.float64)
    if c.epilogue == "clamp":
        y = y.clamp(-1.0, 1.0)
    a = _to_buffer(c, _accumulate(c, d.x.abs(), d.w.abs(), torch.float64), float("nan")) if absacc else None
    return ConvRef(_to_buffer(c, y, float("nan")), a, owned_mask(c))


def round_once_to_bf16(d):
    """float64 -> bf16 with ONE round-to-nearest-even, exactly, in integer arithmetic on the float64 bits (bf16 keeps 7 of
    the 52 fraction bits; a carry out of the fraction moves into the exponent as it should)."""
    mag = d.abs()
    assert bool(((mag == 0) | ((mag >= 2.0 ** -126) & (mag < 2.0 ** 127))).all()), "outside bf16's normal range"
    b = d.contiguous().view(torch.int64)
    r = ((b + ((1 << 44) - 1) + ((b >> 45) & 1)) >> 45) << 45
    return r.view(torch.float64).to(BF16)      # (exact: the value is a bf16 number already)


# ------------------------------------------------------------------------------------------ the norm
def norm_reference(raw_bf16, gamma, C, silu):
    """float64 RMS_norm (vae.py:41-56) + SiLU of bf16 rows [..., C]: u = x sqrt(C) / max(||x||, 1e-12) gamma, SiLU(u) or u.
    Returns (ref, u).

    Bound of check_norm: |got - ref| <= 2^-8 |ref| at every element.  Where it comes from, and what it leaves:
      * The fp32 evaluation in front of the final rounding.  Relative to the value: the sum of C squares, in any order,
        (C + 1) 2^-24 (each square rounded, at most C - 1 additions; all terms positive, so this is relative), halved by
        the square root, which with the division and sqrt(C) adds 3 x 2^-24; two products, 2 x 2^-24: u is within
        (C / 2 + 6) 2^-24 |u|.  SiLU(u) = u / (1 + 2^(-log2(e) u)): its logarithmic derivative times u is
        1 + u (1 - sigmoid(u)), at most 1 + |u| in magnitude (this is the conditioning for negative u, where the result
        decays like e^u), so the error of u arrives multiplied by (1 + |u|); the rounded product log2(e) u moves the
        exponential by |u| 2^-24 relative, exp2 and rcp are 1 ulp instructions, the addition and the last product one
        rounding each: 4 x 2^-24 more.  In all at most (1 + |u|) (C / 2 + 6) 2^-24 + (|u| + 4) 2^-24
        <= (1 + |u|) (C + 10) 2^-24 in the worst case, every rounding pulling the same way.
      * check_norm ASSERTS that its inputs keep (1 + max |u|) (C + 10) 2^-24 below 2^-9, half the bound.
        |u| <= sqrt(C) max |gamma|, so with gamma within 1 +- 0.5 and C <= 512 the left side is at most
        35 x 522 x 2^-24 = 2^-9.8.
      * The final round-to-nearest-even to bf16 (8 significant bits).  Its error is at most 2^-8 of the binade's LOWER
        power of two: 2^-9 of a value just below the next power, but 2^-8 / (1 + 2^-8) of a value just above this one.
        The split "2^-9 for the rounding, 2^-9 for the arithmetic" therefore holds at the top of a binade only; in its
        lowest 1 / 256 the rounding may take all but 2^-16 |ref| of the bound, as in tests/test_gpu_gemm_batched.py.
        2^-16 is 256 fp32 roundings: more than the worst case of the first item only while (1 + |u|) (C + 10) <= 256.
        The roundings of a sum do not all pull one way, though: the fp32 evaluation of this module's emulation, measured
        in front of its final rounding, is within 11 x 2^-24 |ref| on the convolution cases (|u| < 6) and within
        88 x 2^-24 |ref| on the worst rows of the sf_rmsnorm_silu_cl test (C = 512, one dominant element, |u| = 34),
        and a value must sit that close to a rounding tie as well.  The host test measures a worst err / tol of
        0.996 = 1 / (1 + 2^-8) for the emulation: the rounding alone."""
    x, g = raw_bf16.double(), gamma.double()
    nrm = x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
    u = x * math.sqrt(C) / nrm * g
    return (u * torch.sigmoid(u) if silu else u), u


def norm_fp32(raw_bf16, gamma, C, silu, bug=None):
    """The kernels' arithmetic in fp32 torch (rmsnorm_silu_kernel and the halo kernel's fused form)."""
    v, g = raw_bf16.float(), gamma.float()
    ss = (v * v).sum(-1, keepdim=True)
    scale = torch.tensor(float(C if bug != "norm_other_width" else (96 if C == 192 else 192)), dtype=torch.float32).sqrt()
    inv = scale / ss.sqrt().clamp_min(1e-12)
    if bug == "norm_neighbour_row":
        flat = inv.reshape(-1, 1)
        inv = flat[torch.arange(flat.shape[0]) ^ 1].reshape(inv.shape)
    y = v * inv * g
    if silu:
        y = y * (1.0 / (1.0 + torch.exp2(-torch.tensor(LOG2E_F32, dtype=torch.float32) * y)))
    return y.to(BF16)


# ------------------------------------------------------------------------------------------ the emulation and its wrong variants
BUGS = ("drop_corner_tap", "bias_neighbour_group", "resid_next_frame", "ragged_clamped_neighbour", "norm_neighbour_row",
        "norm_other_width", "no_clamp", "interleave_swapped", "upsample_round_up", "stride_pad_left")


def fp32_emulation(c, d, bug=None):
    """{"out": bf16 buffer | "out_f32": float buffer, "norm_out": bf16 buffer} of a correct fp32 implementation, or, with
    `bug` one of BUGS, of a subtly wrong one.  Unowned elements hold NaN."""
    y = _accumulate(c, d.x, d.w, torch.float32, bug)
    bias = d.bias.float()
    if bug == "bias_neighbour_group":
        bias = bias.clone()
        bias[16:32] = d.bias.float()[32:48]
    y = y + bias
    if c.epilogue == "resid":
        y = y + _resid_rows(c, d, torch.float32, bug)
    if bug == "ragged_clamped_neighbour":                      # the last row of a ragged patch taken from the clamped position
        y = y.clone()
        y[:, c.H - 1] = y[:, c.H - 2]
    if c.epilogue == "clamp":
        return {"out_f32": _to_buffer(c, y if bug == "no_clamp" else y.clamp(-1.0, 1.0), float("nan"))}
    raw = y.to(BF16)
    if bug == "interleave_swapped":
        raw = torch.cat([raw[..., c.Cout // 2:], raw[..., :c.Cout // 2]], dim=-1)
    res = {"out": _to_buffer(c, raw, float("nan"))}
    if c.norm:
        n = torch.full(c.norm_shape, float("nan"), dtype=BF16)
        n[c.norm_frame_offset:c.norm_frame_offset + c.T, :, :, :c.Cout] = norm_fp32(raw, d.gamma, c.Cout, True, bug)
        res["norm_out"] = n
    return res


# ------------------------------------------------------------------------------------------ checkers
class Mismatch(AssertionError):
    def __init__(self, msg, index, count, worst):
        super().__init__(msg)
        self.index, self.count, self.worst = index, count, worst


def _report(what, bad, got, want, ratio):
    """Raise for the first bad element of `bad`; ratio: err / tol where that is finite."""
    if not bool(bad.any()):
        return
    idx = tuple(int(v) for v in bad.nonzero()[0])
    fin = ratio[torch.isfinite(ratio)]
    worst = float(fin.max()) if fin.numel() else float("nan")
    raise Mismatch(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first at (t, h, w, n) = {idx}: got {float(got[idx])!r}, "
                   f"want {float(want[idx])!r}; worst err / tol {worst:.3f}", idx, int(bad.sum()), worst)


def check_bits(got, r, what=""):
    """Integer family, bf16: every owned element equals one round-to-nearest-even of the exact value, bit for bit."""
    assert got.dtype == BF16 and got.shape == r.ref.shape
    want = round_once_to_bf16(torch.where(r.owned, r.ref, torch.zeros_like(r.ref)))
    bad = r.owned & (got.view(torch.int16) != want.view(torch.int16))
    ulp = (2.0 ** -8 * want.double().abs()).clamp_min(2.0 ** -133)        # (a bf16 step is at most this)
    _report(what + " [bit-equal]", bad, got, want, torch.where(r.owned, (got.double() - want.double()).abs() / ulp, torch.zeros_like(r.ref)))
    return 0.0


def check_exact_f32(got, r, what=""):
    """Integer family, float head: every owned element equals the clamped exact value."""
    assert got.dtype == torch.float32 and got.shape == r.ref.shape
    bad = r.owned & ~(got.double() == r.ref)
    _report(what + " [fp32-equal]", bad, got, r.ref, torch.where(r.owned, (got.double() - r.ref).abs() / 2.0 ** -24, torch.zeros_like(r.ref)))
    return 0.0


def check_bound(got, r, K, what=""):
    """Gaussian family: the bound of the module docstring at every owned element.  Returns the worst err / tol."""
    assert got.shape == r.ref.shape and r.absacc is not None
    tol = K * 2.0 ** -22 * r.absacc + (2.0 ** -8 if got.dtype == BF16 else 2.0 ** -23) * r.ref.abs()
    err = (got.double() - r.ref).abs()
    bad = r.owned & ~(err <= tol)                  # (a NaN in `got` is bad too)
    ratio = torch.where(r.owned, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    _report(what + " [bound]", bad, got, r.ref, ratio)
    return float(ratio.max())


def check_norm(got, raw_bf16, gamma, C, silu, owned=None, what=""):
    """got, raw: bf16 [..., >= C]; the first C channels of every row with owned[...] (default: all) are compared with
    norm_reference of the raw row.  Returns the worst err / tol."""
    ref, u = norm_reference(raw_bf16[..., :C], gamma, C, silu)
    rows = torch.ones(ref.shape[:-1], dtype=torch.bool) if owned is None else owned
    u_max = float(u[rows].abs().max()) if bool(rows.any()) else 0.0
    assert (1 + u_max) * (C + 10) * 2.0 ** -24 < 2.0 ** -9, f"{what}: max |u| = {u_max} at C = {C} leaves the fp32 evaluation no room"
    g = got[..., :C].double()
    tol = 2.0 ** -8 * ref.abs()
    err = (g - ref).abs()
    bad = rows[..., None] & ~(err <= tol)
    ratio = torch.where(rows[..., None] & (tol > 0), err / tol.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(rows[..., None], ratio, torch.zeros_like(ratio))
    _report(what + " [norm]", bad, g, ref, ratio)
    return float(ratio.max())


def check_case(c, d, r, res, what=""):
    """The checks a launch's outputs get: `res` as fp32_emulation returns it (a missing "out": launched with out = NULL).
    Returns {"conv": worst, "norm": worst} of what was checked."""
    worst = {}
    if "out_f32" in res:
        worst["conv"] = check_exact_f32(res["out_f32"], r, what) if c.family == "int" else check_bound(res["out_f32"], r, c.K, what)
    if "out" in res:
        worst["conv"] = check_bits(res["out"], r, what) if c.family == "int" else check_bound(res["out"], r, c.K, what)
        if "norm_out" in res:
            f0, n0 = c.out_frame_offset, c.norm_frame_offset
            raw = res["out"][f0:f0 + c.T, :, :, :c.Cout]
            worst["norm"] = check_norm(res["norm_out"][n0:n0 + c.T], raw, d.gamma, c.Cout, True, what=what)
    return worst


# ------------------------------------------------------------------------------------------ canaries
def fill_value(dtype):
    v = FILL[dtype]
    return v - (1 << 16) if dtype == torch.bfloat16 and v >= 1 << 15 else v


class Canary:
    """`shape` output elements of `dtype` between two guard bands, all pre-filled with the NaN pattern."""

    def __init__(self, shape, dtype, device="cpu"):
        self.shape, self.dtype = tuple(shape), dtype
        self.n = math.prod(self.shape)
        self.raw = torch.full((self.n + 2 * GUARD,), fill_value(dtype), dtype=INT[dtype], device=device)
        self.region = self.raw[GUARD:GUARD + self.n].view(dtype).view(self.shape)

    def ptr(self):
        return self.region.data_ptr()

    def host(self):
        return self.region.cpu()

    def assert_untouched_outside(self, owned, what="output"):
        """`owned`: bool of the buffer's shape, the elements the launch may write.  Everything else, guard bands included,
        still holds the fill."""
        raw = self.raw.cpu()
        fv = fill_value(self.dtype)
        assert bool((raw[:GUARD] == fv).all()), f"{what}: the guard band in front was written"
        assert bool((raw[GUARD + self.n:] == fv).all()), f"{what}: the guard band behind was written"
        stray = (raw[GUARD:GUARD + self.n].view(self.shape) != fv) & ~owned
        if bool(stray.any()):
            idx = tuple(int(v) for v in stray.nonzero()[0])
            raise AssertionError(f"{what}: {int(stray.sum())} elements the launch does not own were written, first at {idx}")
