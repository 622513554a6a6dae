// gm_shrot.hip -- spherical-harmonics rows re-expressed in another frame (gm_sh_rotate): the colour half of baking an edit into a plain
// Gaussian cloud (deform.rotate_sh, SingleObjectDeform.bake).
//
// The edit path evaluates SH at dir_rot = A^T d (sh_colors_kernel, shade_rotated in gm_deform.hip; A = gm_deform's rot_out, a barycentric
// blend of rotations and NOT orthogonal; d is normalised before A^T is applied).  A plain cloud has no A: its viewer evaluates SH at d.
// The row c' written here gives that viewer the same colour:   SH_deg(d) . c' == SH_deg(A^T d) . c   for every unit d.
// Band l of gm_sh.h's polynomial is homogeneous of degree l in (x, y, z), so the right side is, on the unit sphere, a polynomial of degree
// <= deg: it lies in the span of the same (deg+1)^2 functions, exactly, for ANY 3x3 matrix (bands l, l-2, .. mix when A is not orthogonal).
//
// Method: direction sampling.  The right side is evaluated with sh_channel - the polynomial its consumers evaluate, contraction off - at
// the 32 fixed Fibonacci directions SHROT_DIR, and the samples are multiplied by the pseudo-inverse of the 32 x 16 matrix of the basis at
// those directions (condition number 1.18; SHROT_PINVT is its transpose, tools/sh_rotate_table.py prints both tables).  A degree below
// 3 uses the first (deg+1)^2 weights of each sample: the sampled function has no component in the higher bands.  The products with the
// table accumulate by explicit fmaf in the fixed order j = 0..31: the same bits every run, in place or not.
//
// One thread per row, everything in registers: the row by load_sh's route (16-byte loads when the row stride and the bases allow them,
// one float at a time otherwise), A by nine loads.  The loop over the samples is rolled: its index is wave-uniform, so sample j's
// direction and weights (constant memory, 80 B) come by scalar loads and are scalar operands of the lanes' arithmetic (unrolled, every
// sample was hoisted and 174 VGPRs spilled).  A thread has read its whole row before it writes it, so shs_out == shs is allowed.
// No workspace, no device allocation, no host wait: stream-ordered.
#include "gm_common.h"
#include "gm_check.h"
#pragma clang fp contract(off)
#include "gm_sh.h"

namespace gm {

#define SHROT_K 32
// 32 Fibonacci directions; condition number of the basis matrix 1.176
__constant__ float SHROT_DIR[32][4] = {
    {0.089883171f, -0.231180564f, 0.96875f, 0.0f},
    {-0.379107922f, 0.187051147f, 0.90625f, 0.0f},
    {0.51534456f, 0.150019839f, 0.84375f, 0.0f},
    {-0.324080795f, -0.53349793f, 0.78125f, 0.0f},
    {-0.135224327f, 0.681991816f, 0.71875f, 0.0f},
    {0.608164847f, -0.446622252f, 0.65625f, 0.0f},
    {-0.799943864f, -0.0868951231f, 0.59375f, 0.0f},
    {0.559254825f, 0.636402011f, 0.53125f, 0.0f},
    {0.0182525534f, -0.883142292f, 0.46875f, 0.0f},
    {-0.631028056f, 0.660881579f, 0.40625f, 0.0f},
    {0.936962247f, -0.0627507493f, 0.34375f, 0.0f},
    {-0.749339223f, -0.599490762f, 0.28125f, 0.0f},
    {0.150072485f, 0.964171529f, 0.21875f, 0.0f},
    {0.547243178f, -0.822259605f, 0.15625f, 0.0f},
    {-0.966597199f, 0.238538772f, 0.09375f, 0.0f},
    {0.877306402f, 0.478912234f, 0.03125f, 0.0f},
    {-0.323397875f, -0.945746958f, -0.03125f, 0.0f},
    {-0.398810774f, 0.912228525f, -0.09375f, 0.0f},
    {0.903069139f, -0.400065124f, -0.15625f, 0.0f},
    {-0.924821973f, -0.311211824f, -0.21875f, 0.0f},
    {0.463908821f, 0.84005183f, -0.28125f, 0.0f},
    {0.220543176f, -0.91279608f, -0.34375f, 0.0f},
    {-0.758213937f, 0.509973049f, -0.40625f, 0.0f},
    {0.873473704f, 0.131594434f, -0.46875f, 0.0f},
    {-0.532482505f, -0.658965707f, -0.53125f, 0.0f},
    {-0.0498518087f, 0.803103805f, -0.59375f, 0.0f},
    {0.543177843f, -0.523730636f, -0.65625f, 0.0f},
    {-0.695041835f, 0.0177573785f, -0.71875f, 0.0f},
    {0.470898122f, 0.409760147f, -0.78125f, 0.0f},
    {-0.0605651848f, -0.533308327f, -0.84375f, 0.0f},
    {-0.248560369f, 0.34194836f, -0.90625f, 0.0f},
    {0.243064418f, -0.0494280159f, -0.96875f, 0.0f}};
__constant__ float SHROT_PINVT[32][16] = {
    {0.108852074f, 0.0375775285f, 0.183056116f, -0.0199600514f, -0.0104322005f, 0.0852529854f, 0.219814599f, -0.035097748f, -0.0153322183f, -0.00210548169f, -0.0210342202f, 0.125127599f, 0.236727744f, -0.0664160401f, -0.0434910357f, 0.0125026815f},
    {0.113330632f, -0.0409743823f, 0.174360856f, 0.0692851543f, -0.0268526673f, -0.088773407f, 0.18954055f, 0.138212889f, 0.0223321561f, -0.0231653973f, -0.0653924197f, -0.12117184f, 0.149240881f, 0.196843982f, 0.0650795698f, 0.0106638484f},
    {0.110714674f, -0.0385654643f, 0.176272064f, -0.0981728062f, 0.0353662819f, -0.0694175586f, 0.140366331f, -0.176554456f, 0.0458920449f, -0.030828923f, 0.0931090266f, -0.108573601f, 0.0934334099f, -0.23481445f, 0.0994847119f, -0.0248354319f},
    {0.107406162f, 0.101171128f, 0.13617599f, 0.0590190701f, 0.0712245777f, 0.178259552f, 0.0949210003f, 0.101583488f, -0.0392714962f, 0.0079916399f, 0.13881661f, 0.192565635f, -0.0124645205f, 0.113039844f, -0.0825090855f, -0.0585943162f},
    {0.118960947f, -0.131835744f, 0.149320185f, 0.0214251485f, -0.0354122631f, -0.222874328f, 0.0879142508f, 0.0350140892f, -0.0962504745f, 0.0718004182f, -0.0575880781f, -0.199782372f, -0.0245071016f, 0.0192728769f, -0.180920005f, -0.0376146063f},
    {0.108000211f, 0.0895034373f, 0.118976682f, -0.110268898f, -0.119217426f, 0.130737662f, 0.0293255858f, -0.169433728f, 0.0330742002f, 0.0903024897f, -0.210778892f, 0.103839278f, -0.0979269072f, -0.102343395f, 0.0447669104f, 0.0420770496f},
    {0.106014021f, 0.0152972527f, 0.108796634f, 0.155462891f, 0.028326463f, 0.0227215476f, -0.00084216235f, 0.197301596f, 0.139857009f, 0.0285500772f, 0.0352133848f, 0.0113335708f, -0.114763968f, 0.117011242f, 0.218623146f, 0.110296071f},
    {0.114835665f, -0.126602963f, 0.112953864f, -0.108079284f, 0.156530097f, -0.153209955f, -0.00897383131f, -0.127259195f, -0.0189403966f, -0.0752329677f, 0.21435003f, -0.0647141635f, -0.103649788f, -0.0433080606f, -0.0292747803f, 0.106812239f},
    {0.110732891f, 0.17547518f, 0.0874871463f, -0.005122195f, -0.00842376892f, 0.182966948f, -0.0451060012f, -0.00776253967f, -0.167530835f, -0.150354221f, -0.021690283f, 0.0343641974f, -0.13700141f, -0.0047611082f, -0.203361839f, 0.0115599446f},
    {0.111533351f, -0.123124667f, 0.0760813951f, 0.123561554f, -0.177127406f, -0.107664965f, -0.0633480474f, 0.1052818f, -0.00553777348f, -0.117233135f, -0.191238329f, 0.034918718f, -0.134531379f, -0.013151695f, -6.04075103e-05f, -0.126180604f},
    {0.110162184f, 0.0130748702f, 0.0565004647f, -0.174232095f, -0.023094913f, 0.0110708512f, -0.0813434348f, -0.137197778f, 0.184830815f, 0.0299753398f, -0.0212328788f, 0.00261498336f, -0.136631057f, 0.0881218836f, 0.175314516f, -0.189590216f},
    {0.107551999f, 0.113596708f, 0.0554383211f, 0.1416924f, 0.18867594f, 0.0712134391f, -0.0999452695f, 0.0929565057f, 0.042378284f, 0.183121726f, 0.151941806f, -0.0705840588f, -0.101362385f, -0.0867250636f, 0.027323056f, -0.0985323712f},
    {0.113016754f, -0.182915524f, 0.0398066267f, -0.0294896215f, 0.0600153878f, -0.0848731101f, -0.0992106795f, -0.0193544179f, -0.192002282f, 0.198197767f, 0.0279067382f, 0.137204528f, -0.0913601667f, 0.0191934649f, -0.123488396f, 0.0936592221f},
    {0.11194396f, 0.162439108f, 0.0327287503f, -0.104943328f, -0.193973348f, 0.0595675595f, -0.110895082f, -0.0375768468f, -0.0798675343f, 0.043729607f, -0.0892236382f, -0.112257347f, -0.0654788539f, 0.0824443623f, -0.0317080058f, 0.222253904f},
    {0.107704975f, -0.0460738912f, 0.0228686072f, 0.18652685f, -0.100785427f, -0.00382045796f, -0.129359722f, 0.0470621809f, 0.191285312f, -0.154475138f, -0.0324276239f, 0.0414309502f, -0.0344630219f, -0.162041336f, 0.0459025614f, 0.17307882f},
    {0.111693345f, -0.0903871134f, -0.00143245573f, -0.167676851f, 0.18320173f, -0.00532373041f, -0.122858085f, -0.0140968328f, 0.118129693f, -0.23518303f, 0.00376640353f, 0.0934033915f, -0.0255079344f, 0.161677182f, 0.0261390749f, -0.0173575412f},
    {0.111693352f, 0.180563599f, 0.00143244863f, 0.0606806986f, 0.133251727f, -0.014794874f, -0.122858085f, -0.00285914238f, -0.172515139f, -0.130075753f, 0.00517642684f, -0.175161481f, 0.0255079363f, -0.0646695867f, 0.0258967485f, -0.196704447f},
    {0.107704982f, -0.176027998f, -0.0228686072f, 0.0770013928f, -0.158864811f, 0.0457351021f, -0.129359737f, -0.0117364703f, -0.146662012f, 0.0755129382f, 0.0458919667f, 0.152682662f, 0.0344630219f, -0.0682782754f, 0.0324426219f, -0.219355062f},
    {0.11194396f, 0.0759137347f, -0.0327287465f, -0.17786701f, -0.156179413f, -0.0269445833f, -0.110895082f, 0.0650715157f, 0.140044555f, 0.215277135f, 0.0735183284f, -0.0622394532f, 0.0654788464f, 0.124599501f, -0.0596767329f, -0.0704615638f},
    {0.113016747f, 0.0600450747f, -0.039806623f, 0.175277829f, 0.120673373f, -0.0334502608f, -0.0992106795f, -0.080368638f, 0.16094923f, 0.178571254f, -0.0675331131f, -0.0421553329f, 0.0913601667f, -0.131971225f, -0.107086174f, 0.12714839f},
    {0.107551999f, -0.158885732f, -0.0554383211f, -0.0879560933f, 0.163702041f, 0.103675276f, -0.0999452695f, 0.0544398837f, -0.102937713f, 0.00352492649f, -0.134101883f, 0.0974272788f, 0.101362392f, 0.0548750646f, 0.0764823258f, 0.207917705f},
    {0.110162176f, 0.169500142f, -0.0565004684f, -0.042396713f, -0.0834770277f, -0.133340344f, -0.0813434273f, 0.0341489241f, -0.16651544f, -0.150760472f, 0.078544721f, -0.0872915685f, 0.136631057f, 0.012348556f, 0.158166811f, 0.118803412f},
    {0.111533351f, -0.100921899f, -0.0760813951f, 0.142274082f, -0.16511561f, 0.0855247676f, -0.0633480474f, -0.123941578f, 0.0643554181f, -0.167377979f, 0.180245563f, 0.00704727462f, 0.134531379f, -0.0366417766f, -0.063903369f, -0.0406173281f},
    {0.110732898f, -0.0246731266f, -0.0874871463f, -0.173807397f, 0.0479910523f, 0.0233398508f, -0.0451059975f, 0.181638137f, 0.160730839f, -0.06339138f, -0.0474481694f, -0.00112815935f, 0.137001395f, -0.0346741118f, -0.198935091f, -0.136826739f},
    {0.114835672f, 0.127961233f, -0.112953871f, 0.106467679f, 0.153872341f, -0.1513706f, -0.00897382665f, -0.129441634f, -0.0344051346f, 0.0564232655f, -0.211824968f, 0.0536433756f, 0.10364978f, 0.0564437918f, 0.043967355f, -0.117835768f},
    {0.106014028f, -0.155807674f, -0.108796634f, 0.0112554822f, -0.0199911725f, 0.198299363f, -0.000842155132f, -0.0110249445f, -0.141289502f, 0.110180706f, 0.0397960953f, -0.117240243f, 0.114763953f, 0.00864910241f, 0.21783556f, -0.0289921127f},
    {0.108000211f, 0.0935159326f, -0.118976682f, -0.106887162f, -0.123419225f, -0.14484182f, 0.0293255877f, 0.157546744f, 0.00862514786f, 0.0808404908f, 0.2136309f, 0.0832767934f, 0.0979269147f, -0.119673483f, -0.0281718541f, 0.0582222678f},
    {0.118960947f, 0.00121424638f, -0.149320185f, 0.133559823f, -0.00124645082f, -0.00324141583f, 0.0879142508f, -0.225584671f, 0.102550611f, 0.00227118051f, -0.00611768616f, 0.0148439491f, 0.0245071109f, 0.200160176f, -0.189765662f, 0.0810246915f},
    {0.107406162f, -0.0753023177f, -0.13617599f, -0.0897129327f, 0.0802490488f, 0.130308673f, 0.0949209929f, 0.158478141f, 0.013239353f, -0.0472155288f, -0.158398092f, -0.144022614f, 0.0124645326f, -0.170637086f, -0.0314299874f, 0.0356069356f},
    {0.110714674f, 0.103286423f, -0.176272064f, 0.0213801209f, 0.0180156697f, -0.185761184f, 0.140366346f, -0.0385104679f, -0.0550662205f, -0.0367336832f, -0.0545530133f, 0.249811515f, -0.0934334248f, 0.0672328994f, 0.124861799f, -0.0147600239f},
    {0.113330632f, -0.0613440089f, -0.174360856f, 0.0521176159f, -0.0327677242f, 0.121179834f, 0.189540535f, -0.11090073f, -0.0120858457f, -0.00201699673f, 0.0833677575f, -0.173476264f, -0.149240896f, 0.152761757f, 0.039513763f, -0.0254221316f},
    {0.108852066f, 0.0133069213f, -0.183056101f, -0.0404153466f, -0.00471486198f, -0.0201508179f, 0.219814599f, 0.0899659395f, 0.0179353766f, 0.00987911131f, 0.00530752959f, 0.0442627929f, -0.236727729f, -0.134568989f, -0.0480181128f, -0.00794690289f}};

// row i: coefficients k < (DEG+1)^2 re-expressed, the rest of the row copied when the output is another buffer
template <int DEG>
__global__ __launch_bounds__(256) void sh_rotate_kernel(int N, int M, const float* shs, const float* __restrict__ rot, float* shs_out) {
  constexpr int NC = (DEG + 1) * (DEG + 1), NF = 3 * NC, NQ = (NF + 3) / 4;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const size_t row = (size_t)i * (size_t)M * 3;
  // 16-byte accesses: load_sh's condition on the input, and the same of the output
  const bool vec = (((size_t)M * 3) & 3) == 0 && ((reinterpret_cast<uintptr_t>(shs) | reinterpret_cast<uintptr_t>(shs_out)) & 15) == 0;
  float sh[48];
  load_sh(shs, (size_t)i, M, NC, sh);              // (vec: whole granules, so sh[NF .. 4 NQ) holds the input's next coefficients)
  float A[9];
#pragma unroll
  for (int k = 0; k < 9; k++) A[k] = rot[9 * (size_t)i + k];
  float acc[NF];
#pragma unroll
  for (int k = 0; k < NF; k++) acc[k] = 0.f;
#pragma unroll 1
  for (int j = 0; j < SHROT_K; j++) {              // rolled: j is wave-uniform, so sample j's direction and weights come by scalar loads
    const float dx = SHROT_DIR[j][0], dy = SHROT_DIR[j][1], dz = SHROT_DIR[j][2];
    // dir_rot = A^T d, as sh_colors_kernel forms it
    const float x = (A[0] * dx + A[3] * dy) + A[6] * dz;
    const float y = (A[1] * dx + A[4] * dy) + A[7] * dz;
    const float z = (A[2] * dx + A[5] * dy) + A[8] * dz;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
      const float f = sh_channel(DEG, [&](int k) { return sh[3 * k + ch]; }, x, y, z);
#pragma unroll
      for (int k = 0; k < NC; k++) acc[3 * k + ch] = fmaf(SHROT_PINVT[j][k], f, acc[3 * k + ch]);
    }
  }
#pragma unroll
  for (int k = 0; k < NF; k++) sh[k] = acc[k];
  const int nf_row = M * 3;
  if (vec) {
    float4* o4 = reinterpret_cast<float4*>(shs_out + row);
#pragma unroll
    for (int q = 0; q < NQ; q++) o4[q] = make_float4(sh[4 * q], sh[4 * q + 1], sh[4 * q + 2], sh[4 * q + 3]);
    if (shs_out != shs) {
      const float4* i4 = reinterpret_cast<const float4*>(shs + row);
      for (int q = NQ; 4 * q < nf_row; q++) o4[q] = i4[q];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NF; k++) shs_out[row + k] = sh[k];
    if (shs_out != shs)
      for (int k = NF; k < nf_row; k++) shs_out[row + k] = shs[row + k];
  }
}

// degree 0 into another buffer: the rows as they are
__global__ __launch_bounds__(256) void sh_rotate_copy_kernel(size_t n, const float* __restrict__ shs, float* __restrict__ shs_out) {
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (size_t)gridDim.x * 256) shs_out[k] = shs[k];
}

}  // namespace gm

// ---------------------------------------------------------------------------------------------
// the entry points (include/gmesh_hip.h): their refusals, then the launches
using namespace gm;

extern "C" {

int gm_sh_rotate(int N, int deg, int M, const float* shs, const float* rot, float* shs_out, void* stream) {
  const char* fn = "gm_sh_rotate";
  if (N < 0) { set_error("%s: negative N = %d", fn, N); return GM_ERR_INVALID_ARG; }
  if (N == 0) return GM_OK;
  if (deg < 0 || deg > 3) { set_error("%s: degree %d out of range 0..3", fn, deg); return GM_ERR_INVALID_ARG; }
  if (M < (deg + 1) * (deg + 1)) { set_error("%s: rows of M = %d coefficients hold no degree %d", fn, M, deg); return GM_ERR_INVALID_ARG; }
  if (!shs || !rot || !shs_out) { set_error("%s: null pointer", fn); return GM_ERR_INVALID_ARG; }
  const size_t n = (size_t)N * (size_t)M * 3;
  // shs_out == shs is the in-place call: shs is then left out; any other meeting of the two is an overlap
  const ByteRange rg[3] = {{shs_out, 4 * n, "shs_out", true}, {shs_out == shs ? nullptr : shs, 4 * n, "shs", false}, {rot, 36 * (size_t)N, "rot", false}};
  if (int rc = check_ranges(fn, rg)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((N + 255) / 256), block(256);
  if (deg == 0) {
    const size_t blocks = (n + 255) / 256;
    if (shs_out != shs) hipLaunchKernelGGL(sh_rotate_copy_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), block, 0, s, n, shs, shs_out);
  } else if (deg == 1) {
    hipLaunchKernelGGL(sh_rotate_kernel<1>, grid, block, 0, s, N, M, shs, rot, shs_out);
  } else if (deg == 2) {
    hipLaunchKernelGGL(sh_rotate_kernel<2>, grid, block, 0, s, N, M, shs, rot, shs_out);
  } else {
    hipLaunchKernelGGL(sh_rotate_kernel<3>, grid, block, 0, s, N, M, shs, rot, shs_out);
  }
  GM_HIP(hipGetLastError());
  return GM_OK;
}

}  // extern "C"
