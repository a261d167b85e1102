// C++ driver program over the operator part of include/mugiq_hip_operators.hpp: every wrapper and class the header declares is EXECUTED
// here -- beside what tests/cpp/loop.cpp runs of the loop classes, and with the loop-level wrappers and members that program leaves out
// (the last step) -- on the device buffers the Python tests wrote, so that
// tests/test_gpu_cpp_operators.py can hold what a C++ host gets to what the Python binding gets from the same bytes, bit for bit.
//
//   operators_cpp_test DIR           read DIR/manifest.txt (tests/cpp_exchange.py), upload every buffer, run the steps below through the
//                                    header's wrappers, write DIR/results.txt and one raw file per output buffer
//   operators_cpp_test --list        the header names the program executes, one per line (no GPU)
//   operators_cpp_test --host-selftest   detail::mgOutputs / mgHistory / mgLevels and the dense host helpers (no GPU)
//   operators_cpp_test --parse-only DIR  read DIR/manifest.txt, write the descriptors back to DIR/manifest.out.txt (no GPU)
//
// The first failed HIP call or unexpected exception ends the program with a non-zero exit code; nothing is started after it.
#include <hip/hip_runtime.h>

#include <cinttypes>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <limits>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "mugiq_hip_operators.hpp"

using namespace mugiq_hip;
typedef std::complex<double> cplx;

static const char *EXECUTED[] = {
    "Error", "check", "precisionOf", "deflateLowModes", "restrictVecs", "restrictCoarseVecs", "deflateLowModesCoarse", "wilsonApply", "computeEvals",
    "computeEvalsCoarse", "CoarseOperator", "CoarseOperator::desc", "computeCoarseOperator", "computeCoarseOperatorCoarse", "setCoarseVectors",
    "getCoarseVector", "coarseApply", "coarseApplyForm", "projectVector", "MgSolveParam", "mgPrecondition", "mgSolve", "mgPreconditionSloppy",
    "mgSolveMixed", "mgConvertPrecision", "transferConvert", "blockOrthonormalize", "transferOrthonormality", "MgSetupParam", "mgSetup", "coarseGram",
    "coarseRotate", "hermitianEigh", "choleskyUpper", "upperTriangularInverse", "CoarseEigParam", "coarseEigensolve", "wilsonSolve",
    "exchangeExtendedGauge", "stoutSmear", "plaquette", "CloverField", "CloverField::compute", "CloverField::desc", "CloverField::bytes",
    "Eigsolve_Mugiq", "Eigsolve_Mugiq::computeEvals", "Eigsolve_Mugiq::computeEvecs", "Eigsolve_Mugiq::getCoarseEvecs", "Eigsolve_Mugiq::printEvals",
    "Eigsolve_Mugiq::projectVector", "Eigsolve_Mugiq::solve", "Eigsolve_Mugiq::getEvecs", "Eigsolve_Mugiq::getEvals", "Eigsolve_Mugiq::getEvalsQuda",
    "Eigsolve_Mugiq::getEvalsRes", "Eigsolve_Mugiq::getEvalsSigma", "fusedForm", "transferForm",
    // the loop level, where tests/cpp/loop.cpp does not go
    "checkField", "copyGammaCoeffStructToSymbol", "copyGammaMapStructToSymbol", "GammaName", "performLoopContractionBatched", "createPhaseMatrixGPU",
    "convertIdxOrder_mapGamma", "momentumProjectionGemm", "computeLoop", "MugiqLoopParam", "setDisplaceEntryString", "Loop_Mugiq",
    "Loop_Mugiq::computeCoarseLoop", "Loop_Mugiq::dataPos", "Loop_Mugiq::dataPos_d", "Loop_Mugiq::entryKernel", "Loop_Mugiq::info", "Loop_Mugiq::deflate",
    "Loop_Mugiq::deflateCoarse", "Displace", "Displace::setupDisplacement", "Displace::dir", "Displace::sign", "Displace::gauge",
    "Displace::resetAuxDispVec", "Displace::swapAuxDispVec", "Displace::WhichDisplaceFlag", "Displace::WhichDisplaceDir", "Displace::WhichDisplaceSign",
    "Displace::doVectorDisplacement", "exchangeGhostVec", "performCovariantDisplacementVector"};

[[noreturn]] static void die(int code, const std::string &what) {
  fprintf(stderr, "operators_cpp_test: %s\n", what.c_str());
  fflush(nullptr);
  _Exit(code);  // no destructor and no further GPU call runs after a failure
}
#define HIPX(x)                                                                      \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) die(3, std::string(#x) + " failed: " + hipGetErrorString(e_)); \
  } while (0)

// ---- the manifest (tests/cpp_exchange.py) --------------------------------------------------------------------------------------------
struct Obj {
  std::string kind, name, file = "-";
  int precision = 8, order = 2, X[4] = {0, 0, 0, 0}, R[4] = {0, 0, 0, 0}, volumeCB = 0, stride = 0, nVec = 0, geo[4] = {0, 0, 0, 0}, spinBlockSize = 0;
  int nSpin = 0, nColor = 0, hasClover = 0;
  int64_t parity_offset = 0;
  double kappa = 0.0;
  std::vector<double> values;
  void *d = nullptr;
};

static void ints4(const std::string &v, int out[4]) {
  if (sscanf(v.c_str(), "%d,%d,%d,%d", &out[0], &out[1], &out[2], &out[3]) != 4) die(2, "manifest: four integers expected in " + v);
}
static std::string join4(const int v[4]) {
  char b[96];
  snprintf(b, sizeof b, "%d,%d,%d,%d", v[0], v[1], v[2], v[3]);
  return b;
}
static std::string hexd(double v) {
  char b[64];
  snprintf(b, sizeof b, "%a", v);
  return b;
}

static Obj parseLine(const std::string &text) {
  std::istringstream in(text);
  Obj o;
  in >> o.kind;
  std::string tok;
  while (in >> tok) {
    const size_t eq = tok.find('=');
    if (eq == std::string::npos) die(2, "manifest: token without '=': " + tok);
    const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
    if (k == "name") o.name = v;
    else if (k == "file") o.file = v;
    else if (k == "precision") o.precision = atoi(v.c_str());
    else if (k == "order") o.order = atoi(v.c_str());
    else if (k == "X") ints4(v, o.X);
    else if (k == "R") ints4(v, o.R);
    else if (k == "geoBlockSize") ints4(v, o.geo);
    else if (k == "volumeCB") o.volumeCB = atoi(v.c_str());
    else if (k == "stride") o.stride = atoi(v.c_str());
    else if (k == "parity_offset") o.parity_offset = strtoll(v.c_str(), nullptr, 10);
    else if (k == "nVec") o.nVec = atoi(v.c_str());
    else if (k == "spinBlockSize") o.spinBlockSize = atoi(v.c_str());
    else if (k == "nSpin") o.nSpin = atoi(v.c_str());
    else if (k == "nColor") o.nColor = atoi(v.c_str());
    else if (k == "hasClover") o.hasClover = atoi(v.c_str());
    else if (k == "kappa") o.kappa = strtod(v.c_str(), nullptr);
    else if (k == "values") {
      if (v != "-") {
        std::istringstream vs(v);
        std::string one;
        while (std::getline(vs, one, ',')) o.values.push_back(strtod(one.c_str(), nullptr));
      }
    } else die(2, "manifest: unknown key " + k);
  }
  return o;
}

static std::string formatLine(const Obj &o) {
  std::ostringstream s;
  s << o.kind << " name=" << o.name;
  if (o.kind != "scalars") s << " file=" << o.file;
  const std::string po = " parity_offset=" + std::to_string((long long)o.parity_offset);
  if (o.kind == "spinor")
    s << " precision=" << o.precision << " order=" << o.order << " X=" << join4(o.X) << " volumeCB=" << o.volumeCB << " stride=" << o.stride << po;
  else if (o.kind == "coarse")
    s << " precision=" << o.precision << " nSpin=" << o.nSpin << " nColor=" << o.nColor << " X=" << join4(o.X) << " volumeCB=" << o.volumeCB
      << " stride=" << o.stride << po;
  else if (o.kind == "gauge") s << " precision=" << o.precision << " X=" << join4(o.X) << " R=" << join4(o.R) << " stride=" << o.stride << po;
  else if (o.kind == "clover") s << " precision=" << o.precision << " X=" << join4(o.X) << " volumeCB=" << o.volumeCB << " stride=" << o.stride << po;
  else if (o.kind == "transfer")
    s << " precision=" << o.precision << " nVec=" << o.nVec << " geoBlockSize=" << join4(o.geo) << " spinBlockSize=" << o.spinBlockSize
      << " X=" << join4(o.X) << " stride=" << o.stride << po;
  else if (o.kind == "coarseop")
    s << " precision=" << o.precision << " nVec=" << o.nVec << " X=" << join4(o.X) << " volumeCB=" << o.volumeCB << " kappa=" << hexd(o.kappa)
      << " hasClover=" << o.hasClover;
  else if (o.kind == "scalars") {
    s << " values=";
    if (o.values.empty()) s << "-";
    for (size_t i = 0; i < o.values.size(); i++) s << (i ? "," : "") << hexd(o.values[i]);
  } else die(2, "manifest: unknown kind " + o.kind);
  return s.str();
}

static std::vector<Obj> readManifest(const std::string &dir) {
  std::ifstream f(dir + "/manifest.txt");
  if (!f) die(2, "cannot open " + dir + "/manifest.txt");
  std::vector<Obj> out;
  std::string text;
  while (std::getline(f, text))
    if (text.find_first_not_of(" \t\r") != std::string::npos) out.push_back(parseLine(text));
  return out;
}

static size_t bytesOf(const Obj &o) {
  const size_t cplxBytes = 2 * (size_t)o.precision;
  if (o.kind == "coarseop") return (size_t)2 * o.volumeCB * 9 * (2 * o.nVec) * (2 * o.nVec) * cplxBytes;
  return (size_t)2 * (size_t)o.parity_offset * cplxBytes;
}

// ---- descriptors ---------------------------------------------------------------------------------------------------------------------
static ColorSpinorField asSpinor(const Obj &o) {
  ColorSpinorField f{};
  f.data = o.d; f.precision = o.precision; f.field_order = o.order; f.nParity = 2; f.volumeCB = o.volumeCB; f.stride = o.stride;
  f.parity_offset = o.parity_offset;
  for (int d = 0; d < 4; d++) f.X[d] = o.X[d];
  return f;
}
static MugiqHipCoarseField asCoarse(const Obj &o) {
  MugiqHipCoarseField f{};
  f.data = o.d; f.precision = o.precision; f.nSpin = o.nSpin; f.nColor = o.nColor; f.volumeCB = o.volumeCB; f.stride = o.stride;
  f.parity_offset = o.parity_offset;
  for (int d = 0; d < 4; d++) f.X[d] = o.X[d];
  return f;
}
static GaugeField asGauge(const Obj &o) {
  GaugeField g{};
  g.data = o.d; g.precision = o.precision; g.stride = o.stride; g.parity_offset = o.parity_offset;
  for (int d = 0; d < 4; d++) { g.X[d] = o.X[d]; g.R[d] = o.R[d]; }
  return g;
}
static MugiqHipCloverField asClover(const Obj &o) {
  MugiqHipCloverField c{};
  c.data = o.d; c.precision = o.precision; c.volumeCB = o.volumeCB; c.stride = o.stride; c.parity_offset = o.parity_offset;
  for (int d = 0; d < 4; d++) c.X[d] = o.X[d];
  return c;
}
static MugiqHipTransfer asTransfer(const Obj &o) {
  MugiqHipTransfer t{};
  t.V = o.d; t.precision = o.precision; t.nVec = o.nVec; t.spinBlockSize = o.spinBlockSize; t.stride = o.stride; t.parity_offset = o.parity_offset;
  for (int d = 0; d < 4; d++) { t.X[d] = o.X[d]; t.geoBlockSize[d] = o.geo[d]; }
  return t;
}

// ---- the case: inputs by name, outputs in the order they were made ---------------------------------------------------------------------
struct Case {
  std::string dir;
  std::map<std::string, Obj> in;
  std::vector<Obj> out;
  FILE *res = nullptr;

  const Obj &get(const std::string &name, const char *kind) const {
    auto it = in.find(name);
    if (it == in.end() || it->second.kind != kind) die(2, "manifest: no " + std::string(kind) + " named " + name);
    return it->second;
  }
  ColorSpinorField F(const std::string &n) const { return asSpinor(get(n, "spinor")); }
  std::vector<ColorSpinorField> Fs(const std::string &prefix, int first, int n) const {
    std::vector<ColorSpinorField> v;
    for (int i = first; i < first + n; i++) v.push_back(F(prefix + std::to_string(i)));
    return v;
  }
  MugiqHipCoarseField C(const std::string &n) const { return asCoarse(get(n, "coarse")); }
  std::vector<MugiqHipCoarseField> Cs(const std::string &prefix, int first, int n) const {
    std::vector<MugiqHipCoarseField> v;
    for (int i = first; i < first + n; i++) v.push_back(C(prefix + std::to_string(i)));
    return v;
  }
  GaugeField G(const std::string &n) const { return asGauge(get(n, "gauge")); }
  MugiqHipCloverField Cl(const std::string &n) const { return asClover(get(n, "clover")); }
  MugiqHipTransfer T(const std::string &n) const { return asTransfer(get(n, "transfer")); }
  const std::vector<double> &S(const std::string &n) const { return get(n, "scalars").values; }
  std::vector<cplx> Z(const std::string &n) const {
    const std::vector<double> &v = S(n);
    std::vector<cplx> z(v.size() / 2);
    for (size_t i = 0; i < z.size(); i++) z[i] = cplx(v[2 * i], v[2 * i + 1]);
    return z;
  }

  // a new device buffer described by `o` (kind and geometry), every byte of it `fill`ed: zero, or NaN in the buffer's precision
  Obj &make(Obj o, const std::string &name, bool nan) {
    o.name = name;
    o.file = name + ".out";
    const size_t nb = bytesOf(o);
    HIPX(hipMalloc(&o.d, nb));
    if (nan) {
      if (o.precision == 8) {
        std::vector<double> h(nb / 8, std::numeric_limits<double>::quiet_NaN());
        HIPX(hipMemcpy(o.d, h.data(), nb, hipMemcpyHostToDevice));
      } else {
        std::vector<float> h(nb / 4, std::numeric_limits<float>::quiet_NaN());
        HIPX(hipMemcpy(o.d, h.data(), nb, hipMemcpyHostToDevice));
      }
    } else HIPX(hipMemset(o.d, 0, nb));
    out.push_back(o);
    return out.back();
  }
  // an output that lives in memory somebody else owns (a CoarseOperator, a CloverField, an input updated in place): a copy of it as it
  // is now, since the owner may be gone when the outputs are written
  void keep(const Obj &o, const std::string &name, const void *d) {
    Obj &made = make(o, name, false);
    HIPX(hipMemcpy(made.d, d, bytesOf(made), hipMemcpyDeviceToDevice));
  }
  // fine fields laid out like `like` in `precision`, NaN everywhere (pads included)
  std::vector<ColorSpinorField> newF(const std::string &name, int n, const std::string &like, int precision = 8) {
    std::vector<ColorSpinorField> v;
    for (int i = 0; i < n; i++) {
      Obj o = get(like, "spinor");
      o.precision = precision;
      v.push_back(asSpinor(make(o, name + std::to_string(i), true)));
    }
    return v;
  }
  // copies of input fields: what a call updates in place
  std::vector<ColorSpinorField> copyF(const std::string &name, const std::string &prefix, int first, int n) {
    std::vector<ColorSpinorField> v;
    for (int i = 0; i < n; i++) {
      const Obj &src = get(prefix + std::to_string(first + i), "spinor");
      Obj &o = make(src, name + std::to_string(i), false);
      HIPX(hipMemcpy(o.d, src.d, bytesOf(src), hipMemcpyDeviceToDevice));
      v.push_back(asSpinor(o));
    }
    return v;
  }
  // coarse fields on the lattice X with nColor colours, pad 0, zero
  std::vector<MugiqHipCoarseField> newC(const std::string &name, int n, const int X[4], int nColor, int precision = 8) {
    std::vector<MugiqHipCoarseField> v;
    for (int i = 0; i < n; i++) {
      Obj o;
      o.kind = "coarse"; o.precision = precision; o.nSpin = 2; o.nColor = nColor;
      for (int d = 0; d < 4; d++) o.X[d] = X[d];
      o.volumeCB = X[0] * X[1] * X[2] * X[3] / 2;
      o.stride = o.volumeCB;
      o.parity_offset = (int64_t)2 * nColor * o.stride;
      v.push_back(asCoarse(make(o, name + std::to_string(i), false)));
    }
    return v;
  }
  MugiqHipTransfer newT(const std::string &name, const std::string &like, int precision, bool copy) {
    const Obj &src = get(like, "transfer");
    Obj o = src;
    o.precision = precision;
    Obj &made = make(o, name, false);
    if (copy) HIPX(hipMemcpy(made.d, src.d, bytesOf(src), hipMemcpyDeviceToDevice));
    return asTransfer(made);
  }
  void keepOp(const std::string &name, const CoarseOperator &op) {
    const MugiqHipCoarseOperator &c = *op.desc();
    Obj o;
    o.kind = "coarseop"; o.precision = c.precision; o.nVec = c.nVec; o.volumeCB = c.volumeCB; o.kappa = c.kappa; o.hasClover = c.hasClover;
    for (int d = 0; d < 4; d++) o.X[d] = c.X[d];
    keep(o, name, c.data);
  }

  void putD(const std::string &name, const double *v, size_t n) {
    fprintf(res, "d %s", name.c_str());
    for (size_t i = 0; i < n; i++) fprintf(res, " %a", v[i]);
    fprintf(res, "\n");
  }
  void putD(const std::string &name, const std::vector<double> &v) { putD(name, v.data(), v.size()); }
  void putD(const std::string &name, double v) { putD(name, &v, 1); }
  void putZ(const std::string &name, const std::vector<cplx> &v) { putD(name, reinterpret_cast<const double *>(v.data()), 2 * v.size()); }
  void putI(const std::string &name, const std::vector<long long> &v) {
    fprintf(res, "i %s", name.c_str());
    for (long long x : v) fprintf(res, " %lld", x);
    fprintf(res, "\n");
  }
  void putI(const std::string &name, const std::vector<int> &v) { putI(name, std::vector<long long>(v.begin(), v.end())); }
  void putI(const std::string &name, long long v) { putI(name, std::vector<long long>{v}); }
  void putS(const std::string &name, const std::string &text) {
    fprintf(res, "s %s ", name.c_str());
    for (unsigned char ch : text) fprintf(res, "%02x", ch);
    fprintf(res, "\n");
  }
  // an MG solve's outputs under one name
  void putSolve(const std::string &name, bool ok, const std::vector<int> &iters, const std::vector<double> &relres,
                const std::vector<std::vector<double>> *history, const int *hostReads) {
    putI(name + ".ok", ok ? 1 : 0);
    putI(name + ".iters", iters);
    putD(name + ".relres", relres);
    if (history) {
      putI(name + ".nhist", (long long)history->size());
      for (size_t r = 0; r < history->size(); r++) putD(name + ".hist" + std::to_string(r), (*history)[r]);
    }
    if (hostReads) putI(name + ".hostReads", *hostReads);
  }
  // a call that must throw mugiq_hip::Error: its status and text (status -1: it did not throw)
  void expectError(const std::string &name, const std::function<void()> &call) {
    try {
      call();
      putI(name + ".status", -1);
      putS(name + ".what", "");
    } catch (const Error &e) {
      putI(name + ".status", e.status);
      putS(name + ".what", e.what());
    }
  }

  void load() {
    for (Obj &o : readManifestInto())
      if (o.kind != "scalars" && o.file != "-") {
        const size_t nb = bytesOf(o);
        std::vector<char> h(nb);
        FILE *f = fopen((dir + "/" + o.file).c_str(), "rb");
        if (!f || fread(h.data(), 1, nb, f) != nb || fgetc(f) != EOF) die(2, "manifest: " + o.file + " does not hold the " + std::to_string(nb) + " bytes of its descriptor");
        fclose(f);
        HIPX(hipMalloc(&o.d, nb));
        HIPX(hipMemcpy(o.d, h.data(), nb, hipMemcpyHostToDevice));
        in[o.name] = o;
      } else in[o.name] = o;
  }
  std::vector<Obj> manifest_;
  std::vector<Obj> &readManifestInto() {
    manifest_ = readManifest(dir);
    return manifest_;
  }
  void writeOutputs() {
    HIPX(hipDeviceSynchronize());
    for (const Obj &o : out) {
      const size_t nb = bytesOf(o);
      std::vector<char> h(nb);
      HIPX(hipMemcpy(h.data(), o.d, nb, hipMemcpyDeviceToHost));
      FILE *f = fopen((dir + "/" + o.file).c_str(), "wb");
      if (!f || fwrite(h.data(), 1, nb, f) != nb) die(2, "cannot write " + o.file);
      fclose(f);
      fprintf(res, "buf %s\n", formatLine(o).c_str());
    }
  }
};

static std::vector<MugiqHipCoarseField> head(const std::vector<MugiqHipCoarseField> &v, size_t n) { return std::vector<MugiqHipCoarseField>(v.begin(), v.begin() + n); }
static std::vector<ColorSpinorField> head(const std::vector<ColorSpinorField> &v, size_t n) { return std::vector<ColorSpinorField>(v.begin(), v.begin() + n); }

static void putParam(Case &c, const std::string &name, const MugiqHipMgSolveParam &p) {
  c.putD(name + ".d", std::vector<double>{p.tol, p.omega});
  c.putI(name + ".i", std::vector<int>{p.maxIter, p.nKrylov, p.nuPre, p.nuPost, p.coarseIters});
}
static MgSolveParam solveParam(int nKrylov, int nuPre, int nuPost, int coarseIters, double omega = 1.0) {
  MgSolveParam p;
  p.nKrylov = nKrylov; p.nuPre = nuPre; p.nuPost = nuPost; p.coarseIters = coarseIters; p.omega = omega;
  return p;
}
static void putEigInfo(Case &c, const std::string &name, const MugiqHipCoarseEigInfo &i) {
  c.putI(name + ".i", std::vector<int>{i.iters, i.nConverged, i.opBlocks, i.hostReads});
  c.putD(name + ".d", std::vector<double>{i.aMaxUsed, i.aMinLast, i.orthonormality});  // hostDenseSeconds is a wall time
}
static void putEvals(Case &c, const std::string &name, const std::vector<cplx> &lambda, const std::vector<double> &residual, const std::vector<double> &sigma) {
  c.putZ(name + ".lambda", lambda);
  c.putD(name + ".residual", residual);
  c.putD(name + ".sigma", sigma);
}
static std::string printed(const Eigsolve_Mugiq &es, const std::string &path) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) die(2, "cannot write " + path);
  es.printEvals(f);
  fclose(f);
  std::ifstream in(path);
  std::stringstream s;
  s << in.rdbuf();
  return s.str();
}

// ---- the steps -----------------------------------------------------------------------------------------------------------------------
static void run(Case &c) {
  const int M = MUGIQ_HIP_EIG_OPERATOR_M, MDAGM = MUGIQ_HIP_EIG_OPERATOR_MDAGM, H = EIG_OPERATOR_H;
  const GaugeField Hg = c.G("H.gauge");
  const MugiqHipCloverField Hcl = c.Cl("H.clover");
  const MugiqHipTransfer HT0 = c.T("H.T0"), HT1 = c.T("H.T1");
  const double kappa = c.S("H.kappa")[0], coeff = c.S("H.coeff")[0];
  const std::vector<ColorSpinorField> r = c.Fs("r", 0, 9);
  const std::vector<MugiqHipCoarseField> w = c.Cs("H.w", 0, 9);
  int X1[4], X2[4];
  for (int d = 0; d < 4; d++) {
    X1[d] = HT0.X[d] / HT0.geoBlockSize[d];
    X2[d] = HT1.X[d] / HT1.geoBlockSize[d];
  }
  std::vector<cplx> lambda;
  std::vector<double> residual, sigma, sigmaH, sigmaHclover;
  std::vector<int> iters;
  std::vector<double> relres;

  // CloverField
  c.putI("clover.bytes", (long long)CloverField::bytes(Hg.X, 8));
  CloverField clover(Hg.X, 8);
  clover.compute(Hg, coeff);
  {
    const MugiqHipCloverField &cd = *clover.desc();
    Obj o;
    o.kind = "clover"; o.precision = cd.precision; o.volumeCB = cd.volumeCB; o.stride = cd.stride; o.parity_offset = cd.parity_offset;
    for (int d = 0; d < 4; d++) o.X[d] = cd.X[d];
    c.keep(o, "clover.computed", cd.data);
  }

  // gauge: border refresh (the borders arrive as NaN), one spatial stout step, plaquettes
  {
    const GaugeField Gg = c.G("G.gauge");
    exchangeExtendedGauge(Gg);
    c.keep(c.get("G.gauge", "gauge"), "gauge.exchanged", Gg.data);
    Obj &so = c.make(c.get("G.gauge", "gauge"), "gauge.smeared", false);
    const GaugeField smeared = asGauge(so);
    stoutSmear(smeared, Gg, c.S("G.rho")[0], 1);  // smearDims: the default, 3
    const std::array<double, 3> p0 = plaquette(Gg), p1 = plaquette(smeared);
    c.putD("plaquette.in", p0.data(), 3);
    c.putD("plaquette.smeared", p1.data(), 3);
  }

  // wilsonApply: both overloads, the defaults (M, scale 1) and MdagM with a scale
  wilsonApply(c.newF("wa.M.", 3, "r0"), head(r, 3), Hg, kappa);
  wilsonApply(c.newF("wa.MdagM.", 9, "r0"), r, Hg, kappa, MDAGM, 0.75);
  wilsonApply(c.newF("wac.M.", 2, "r0"), head(r, 2), Hg, clover, kappa);
  wilsonApply(c.newF("wac.MdagM.", 2, "r0"), head(r, 2), Hg, clover, kappa, MDAGM, 0.75);

  // computeEvals: the three sigma rules, both overloads
  const std::vector<ColorSpinorField> ev = head(r, 4);
  computeEvals(ev, Hg, kappa, M, false, lambda, residual, sigma);
  putEvals(c, "ce.M", lambda, residual, sigma);
  computeEvals(ev, Hg, kappa, MDAGM, true, lambda, residual, sigma);
  putEvals(c, "ce.MdagM", lambda, residual, sigma);
  computeEvals(ev, Hg, kappa, H, false, lambda, residual, sigmaH);
  putEvals(c, "ce.H", lambda, residual, sigmaH);
  computeEvals(ev, Hg, clover, kappa, M, false, lambda, residual, sigma);
  putEvals(c, "cec.M", lambda, residual, sigma);
  computeEvals(ev, Hg, clover, kappa, H, false, lambda, residual, sigmaHclover);
  putEvals(c, "cec.H", lambda, residual, sigmaHclover);

  // projectVector
  {
    ColorSpinorField out = c.newF("pv.", 1, "r0")[0], in = r[4];
    projectVector(out, in, ev);
  }

  // deflateLowModes: sigma, gamma5 (default) and overlaps; then none of them, dst == src
  {
    std::vector<cplx> overlaps;
    deflateLowModes(c.copyF("dl.a.", "r", 6, 2), c.Fs("r", 4, 2), ev, sigmaH, true, &overlaps);
    c.putZ("dl.a.overlaps", overlaps);
    const std::vector<ColorSpinorField> x = c.copyF("dl.b.", "r", 4, 2);
    deflateLowModes(x, x, ev, {}, false);
    deflateLowModes(c.copyF("dl.c.", "r", 6, 9 - 6), c.Fs("r", 4, 3), ev);  // every default
  }

  // restriction: 9 vectors; gamma5; the second level
  const std::vector<MugiqHipCoarseField> rc = c.newC("rv.", 9, X1, HT0.nVec);
  restrictVecs(rc, r, HT0);
  const std::vector<MugiqHipCoarseField> rc5 = c.newC("rv5.", 2, X1, HT0.nVec);
  restrictVecs(rc5, head(r, 2), HT0, true);
  const std::vector<MugiqHipCoarseField> rcc = c.newC("rcv.", 2, X2, HT1.nVec);
  restrictCoarseVecs(rcc, head(rc, 2), HT1);

  // deflateLowModesCoarse: one transfer (the defaults, with overlaps) and two (sigma, no gamma5)
  {
    std::vector<cplx> overlaps;
    deflateLowModesCoarse(c.copyF("dlc.a.", "r", 6, 2), c.Fs("r", 4, 2), head(rc, 3), {HT0}, {}, true, &overlaps);
    c.putZ("dlc.a.overlaps", overlaps);
    deflateLowModesCoarse(c.copyF("dlc.b.", "r", 6, 2), c.Fs("r", 4, 2), head(w, 3), {HT0, HT1}, c.S("dlc.sigma"), false);
  }

  // wilsonSolve: plain, deflated with the H eigenpairs of the clover operator, and cut off after two iterations
  {
    const double tol = 1e-10;
    bool ok = wilsonSolve(c.newF("ws.plain.", 2, "r0"), c.Fs("r", 4, 2), Hg, kappa, {}, {}, tol, 1000, iters, relres);
    c.putSolve("ws.plain", ok, iters, relres, nullptr, nullptr);
    ok = wilsonSolve(c.newF("ws.defl.", 2, "r0"), c.Fs("r", 4, 2), Hg, clover, kappa, ev, sigmaHclover, tol, 1000, iters, relres);
    c.putSolve("ws.defl", ok, iters, relres, nullptr, nullptr);
    ok = wilsonSolve(c.newF("ws.cut.", 3, "r0"), c.Fs("r", 4, 3), Hg, kappa, {}, {}, tol, 2, iters, relres);
    c.putSolve("ws.cut", ok, iters, relres, nullptr, nullptr);
  }

  // the coarse operators of hierarchy 0
  CoarseOperator op1(X1, HT0.nVec, 8), op1w(X1, HT0.nVec, 8), op2(X2, HT1.nVec, 8);
  computeCoarseOperator(op1, HT0, Hg, &Hcl, kappa);
  computeCoarseOperator(op1w, HT0, Hg, nullptr, kappa);
  computeCoarseOperatorCoarse(op2, HT1, op1);
  c.keepOp("op1", op1);
  c.keepOp("op1w", op1w);
  c.keepOp("op2", op2);
  {
    const std::vector<MugiqHipCoarseField> cols = c.newC("gcv.", HT1.nVec, X1, HT0.nVec);
    for (int j = 0; j < HT1.nVec; j++) getCoarseVector(cols[j], HT1, j);
    setCoarseVectors(c.newT("scv.T", "H.T1", 8, false), cols);
  }
  coarseApply(c.newC("ca.M.", 9, X2, HT1.nVec), w, op2);
  coarseApply(c.newC("ca.MdagM.", 2, X1, HT0.nVec), head(rc, 2), op1, MDAGM, 0.5);
  c.putI("coarseApplyForm", std::vector<int>{coarseApplyForm(*op2.desc(), 9), coarseApplyForm(*op1.desc(), 2)});
  computeEvalsCoarse(head(w, 3), {HT0, HT1}, Hg, &Hcl, kappa, M, false, lambda, residual, sigma);
  putEvals(c, "cec2.M", lambda, residual, sigma);
  computeEvalsCoarse(head(w, 3), {HT0, HT1}, Hg, &Hcl, kappa, MDAGM, false, lambda, residual, sigma);
  putEvals(c, "cec2.MdagM", lambda, residual, sigma);
  computeEvalsCoarse(head(w, 3), op2, H, false, lambda, residual, sigma);
  putEvals(c, "ceo.H", lambda, residual, sigma);
  computeEvalsCoarse(head(w, 3), op2, M, true, lambda, residual, sigma);
  putEvals(c, "ceo.M", lambda, residual, sigma);

  // the fp32 hierarchies, made here
  const MugiqHipTransfer HT0s = c.newT("H.T0s", "H.T0", 4, false);
  transferConvert(HT0s, HT0);
  CoarseOperator op1s(X1, HT0.nVec, 4);
  computeCoarseOperator(op1s, HT0s, Hg, &Hcl, kappa);
  c.keepOp("op1s", op1s);
  const std::vector<ColorSpinorField> r32 = c.newF("r32.", 3, "r0", 4);
  mgConvertPrecision(r32, head(r, 3));

  const GaugeField Sg = c.G("S.gauge");
  const MugiqHipTransfer ST0 = c.T("S.T0"), ST1 = c.T("S.T1");
  const double kappaS = c.S("S.kappa")[0], tolS = c.S("S.tol")[0];
  int SX1[4], SX2[4];
  for (int d = 0; d < 4; d++) {
    SX1[d] = ST0.X[d] / ST0.geoBlockSize[d];
    SX2[d] = ST1.X[d] / ST1.geoBlockSize[d];
  }
  CoarseOperator Sop1(SX1, ST0.nVec, 8), Sop2(SX2, ST1.nVec, 8), Sop1s(SX1, ST0.nVec, 4), Sop2s(SX2, ST1.nVec, 4);
  computeCoarseOperator(Sop1, ST0, Sg, nullptr, kappaS);
  computeCoarseOperatorCoarse(Sop2, ST1, Sop1);
  const MugiqHipTransfer ST0s = c.newT("S.T0s", "S.T0", 4, false), ST1s = c.newT("S.T1s", "S.T1", 4, false);
  transferConvert(ST0s, ST0);
  transferConvert(ST1s, ST1);
  computeCoarseOperator(Sop1s, ST0s, Sg, nullptr, kappaS);
  computeCoarseOperatorCoarse(Sop2s, ST1s, Sop1s);
  c.keepOp("S.op2", Sop2);
  c.keepOp("S.op2s", Sop2s);
  const std::vector<MugiqHipTransfer> STs = {ST0, ST1}, STss = {ST0s, ST1s};
  const std::vector<MugiqHipCoarseOperator> Sops = {*Sop1.desc(), *Sop2.desc()}, Sopss = {*Sop1s.desc(), *Sop2s.desc()};

  // MgSolveParam
  putParam(c, "MgSolveParam", MgSolveParam());

  // the cycle: one level through the scalar overload (default param) and the vector overload; two levels with params[1] set, 9 vectors;
  // a zero vector inside a batch
  const ColorSpinorField zero = c.F("zero");
  mgPrecondition(c.newF("mp.s.", 2, "r0"), head(r, 2), Hg, &Hcl, kappa, HT0, op1);
  mgPrecondition(c.newF("mp.v1.", 2, "r0"), head(r, 2), Hg, &Hcl, kappa, std::vector<MugiqHipTransfer>{HT0}, {*op1.desc()}, {MgSolveParam()});
  std::vector<MgSolveParam> k3 = {solveParam(16, 1, 1, 2), solveParam(16, 1, 1, 8, 0.85)};  // mg_solve3_cases.K3_PARAMS[1]
  mgPrecondition(c.newF("mp.v2.", 9, "r0"), r, Sg, nullptr, kappaS, STs, Sops, k3);
  mgPrecondition(c.newF("mp.zero.", 3, "r0"), {r[0], zero, r[1]}, Sg, nullptr, kappaS, STs, Sops, k3);
  mgPreconditionSloppy(c.newF("mps.s.", 2, "r0", 4), head(r32, 2), Hg, &Hcl, kappa, HT0s, op1s);
  mgPreconditionSloppy(c.newF("mps.v1.", 2, "r0", 4), head(r32, 2), Hg, &Hcl, kappa, std::vector<MugiqHipTransfer>{HT0s}, {*op1s.desc()}, {MgSolveParam()});
  mgPreconditionSloppy(c.newF("mps.v2.", 3, "r0", 4), r32, Sg, nullptr, kappaS, STss, Sopss, k3);

  // the solves
  {
    std::vector<std::vector<double>> history;
    int hostReads = -1;
    const MgSolveParam one = solveParam(4, 1, 2, 4);  // test_one_level_through_the_new_entry_points_is_the_old_call
    const std::vector<ColorSpinorField> b3 = {r[0], zero, r[1]};
    bool ok = mgSolve(c.newF("ms.s.", 3, "r0"), b3, Hg, &Hcl, kappa, HT0, op1, one, iters, relres, &history, &hostReads);
    c.putSolve("ms.s", ok, iters, relres, &history, &hostReads);
    ok = mgSolve(c.newF("ms.v1.", 3, "r0"), b3, Hg, &Hcl, kappa, std::vector<MugiqHipTransfer>{HT0}, {*op1.desc()}, {one}, iters, relres);
    c.putSolve("ms.v1", ok, iters, relres, nullptr, nullptr);
    ok = mgSolveMixed(c.newF("mm.s.", 3, "r0"), b3, Hg, &Hcl, kappa, &Hg, &Hcl, HT0s, op1s, one, iters, relres, &history, &hostReads);
    c.putSolve("mm.s", ok, iters, relres, &history, &hostReads);
    ok = mgSolveMixed(c.newF("mm.v1.", 3, "r0"), b3, Hg, &Hcl, kappa, nullptr, nullptr, std::vector<MugiqHipTransfer>{HT0s}, {*op1s.desc()}, {one}, iters,
                      relres);
    c.putSolve("mm.v1", ok, iters, relres, nullptr, nullptr);

    // two levels on the smooth hierarchy: mg_solve3_cases.SOLVE_PARAMS at the tolerance of its reference solves
    std::vector<MgSolveParam> sp = {solveParam(16, 0, 4, 4), MgSolveParam()};
    sp[0].tol = tolS;
    sp[1].nuPost = 2;
    sp[1].coarseIters = 4;
    const std::vector<ColorSpinorField> b4 = {c.F("S.b0"), c.F("S.b1"), zero, c.F("S.b2")};
    ok = mgSolve(c.newF("ms.v2.", 4, "r0"), b4, Sg, nullptr, kappaS, STs, Sops, sp, iters, relres, &history, &hostReads);
    c.putSolve("ms.v2", ok, iters, relres, &history, &hostReads);
    ok = mgSolveMixed(c.newF("mm.v2.", 4, "r0"), b4, Sg, nullptr, kappaS, nullptr, nullptr, STss, Sopss, sp, iters, relres, &history, &hostReads);
    c.putSolve("mm.v2", ok, iters, relres, &history, &hostReads);
    sp[0].tol = MgSolveParam().tol;
    ok = mgSolve(c.newF("ms.nine.", 9, "r0"), r, Sg, nullptr, kappaS, STs, Sops, sp, iters, relres, &history, &hostReads);
    c.putSolve("ms.nine", ok, iters, relres, &history, &hostReads);
    sp[0].maxIter = 2;
    ok = mgSolve(c.newF("ms.cut.", 3, "r0"), head(r, 3), Sg, nullptr, kappaS, STs, Sops, sp, iters, relres, &history, &hostReads);
    c.putSolve("ms.cut", ok, iters, relres, &history, &hostReads);
    ok = mgSolveMixed(c.newF("mm.cut.", 3, "r0"), head(r, 3), Sg, nullptr, kappaS, &Sg, nullptr, STss, Sopss, sp, iters, relres, &history, &hostReads);
    c.putSolve("mm.cut", ok, iters, relres, &history, &hostReads);
  }

  // the setup: block orthonormalisation, its check, its refusal of two equal columns; mgSetup with and without a coarse operator
  {
    const MugiqHipTransfer Tbo = c.newT("bo.T", "H.T0", 8, true);
    const MugiqHipBlockOrthoInfo info = blockOrthonormalize(Tbo);
    c.putD("bo.minPivotRatio", info.minPivotRatio);
    c.putI("bo.zeroColumns", info.zeroColumns);
    c.putD("bo.orthonormality", transferOrthonormality(Tbo));
    const MugiqHipTransfer Tdup = c.newT("bo.dup.T", "H.Tdup", 8, true);
    c.expectError("bo.dup", [&] { blockOrthonormalize(Tdup, 2, 1e-8); });

    MgSetupParam sp;
    c.putI("MgSetupParam.i", std::vector<int>{sp.setupMaxIter, sp.nBlockOrtho, sp.refineCycles, sp.refineIters});
    c.putD("MgSetupParam.d", std::vector<double>{sp.setupTol, sp.rankTol});
    sp.setupMaxIter = 10;
    CoarseOperator sop(X1, HT0.nVec, 8);
    MugiqHipMgSetupInfo si = mgSetup(c.newT("su.a.T", "H.T0", 8, false), &sop, head(r, HT0.nVec), Hg, &Hcl, kappa, sp);
    c.keepOp("su.a.op", sop);
    c.putI("su.a.i", std::vector<int>{si.cgIters[0], si.cgIters[1], si.cgIters[2], si.cgIters[3], si.zeroColumns, si.hostReads, si.cgHostReadsEstimate});
    c.putD("su.a.d", std::vector<double>{si.minPivotRatio, si.orthonormality});
    si = mgSetup(c.newT("su.b.T", "H.T0", 8, false), nullptr, head(r, HT0.nVec), Hg, nullptr, kappa, sp);
    c.putI("su.b.i", std::vector<int>{si.cgIters[0], si.cgIters[1], si.cgIters[2], si.cgIters[3], si.zeroColumns, si.hostReads, si.cgHostReadsEstimate});
    c.putD("su.b.d", std::vector<double>{si.minPivotRatio, si.orthonormality});
  }

  // the dense helpers and the coarse eigensolver
  const Obj &EopIn = c.get("E.op", "coarseop");
  CoarseOperator Eop(EopIn.X, EopIn.nVec, 8);
  HIPX(hipMemcpy(Eop.desc()->data, EopIn.d, bytesOf(EopIn), hipMemcpyDeviceToDevice));
  Eop.desc()->kappa = EopIn.kappa;
  Eop.desc()->hasClover = EopIn.hasClover;
  const int nConv = 8, nKr = 24;  // coarse_eig_cases.SIZES[0]
  const std::vector<MugiqHipCoarseField> start = c.Cs("E.s", 0, nKr);
  {
    c.putZ("coarseGram", coarseGram(head(w, 3), w));
    coarseRotate(c.newC("cr.", 2, X2, HT1.nVec), head(w, 3), c.Z("cr.Z"));
    std::vector<double> theta;
    std::vector<cplx> Zm, R, Rinv;
    hermitianEigh(5, c.Z("E.H"), theta, Zm);
    c.putD("eigh.theta", theta);
    c.putZ("eigh.Z", Zm);
    choleskyUpper(5, c.Z("E.G"), R);
    upperTriangularInverse(5, R, Rinv);
    c.putZ("chol.R", R);
    c.putZ("chol.Rinv", Rinv);

    CoarseEigParam ep;
    c.putI("CoarseEigParam.i", std::vector<int>{ep.nConv, ep.nKr, ep.maxIter, ep.polyDeg, ep.nOrtho});
    c.putD("CoarseEigParam.d", std::vector<double>{ep.tol, ep.aMin, ep.aMax, ep.rankTol});
    ep.nConv = nConv; ep.nKr = nKr; ep.polyDeg = 20; ep.tol = 1e-10;
    std::vector<double> res, sig;
    MugiqHipCoarseEigInfo info = coarseEigensolve(c.newC("eig.ev.", nConv, EopIn.X, EopIn.nVec), start, Eop, MDAGM, ep, theta, res, sig);
    putEigInfo(c, "eig.info", info);
    c.putD("eig.theta", theta);
    c.putD("eig.residual", res);
    c.putD("eig.sigma", sig);
    ep.maxIter = 1;
    info = coarseEigensolve(c.newC("eig1.ev.", nConv, EopIn.X, EopIn.nVec), start, Eop, MDAGM, ep, theta, res, sig, true);
    putEigInfo(c, "eig1.info", info);
    c.putD("eig1.theta", theta);
    c.expectError("eig1.strict", [&] { coarseEigensolve(c.newC("eig1s.ev.", nConv, EopIn.X, EopIn.nVec), start, Eop, MDAGM, ep, theta, res, sig); });
  }

  // Eigsolve_Mugiq: the three constructors
  {
    Eigsolve_Mugiq esH(ev, Hg, kappa, H);
    esH.computeEvals();
    putEvals(c, "es.H", *esH.getEvals(), *esH.getEvalsRes(), *esH.getEvalsSigma());
    c.putZ("es.H.quda", *esH.getEvalsQuda());
    c.putI("es.H.nEvecs", (long long)esH.getEvecs().size());
    ColorSpinorField out = c.newF("es.pv.", 1, "r0")[0], in = r[4];
    esH.projectVector(out, in);
    bool ok = esH.solve(c.newF("es.solve.", 2, "r0"), c.Fs("r", 4, 2), 1e-10, 1000, iters, relres);
    c.putSolve("es.solve", ok, iters, relres, nullptr, nullptr);
    c.expectError("es.computeEvecs", [&] { esH.computeEvecs({}, {}); });

    Eigsolve_Mugiq esM(head(ev, 3), Hg, kappa, M), esMM(head(ev, 3), Hg, kappa, MDAGM);
    esM.computeEvals();
    esMM.computeEvals();
    putEvals(c, "es.M", *esM.getEvals(), *esM.getEvalsRes(), *esM.getEvalsSigma());
    putEvals(c, "es.MdagM", *esMM.getEvals(), *esMM.getEvalsRes(), *esMM.getEvalsSigma());
    c.putS("es.M.print", printed(esM, c.dir + "/print.M.txt"));
    c.putS("es.MdagM.print", printed(esMM, c.dir + "/print.MdagM.txt"));

    Eigsolve_Mugiq esC(ev, Hg, clover, kappa, H);
    esC.computeEvals();
    putEvals(c, "esc.H", *esC.getEvals(), *esC.getEvalsRes(), *esC.getEvalsSigma());
    ok = esC.solve(c.newF("esc.solve.", 2, "r0"), c.Fs("r", 4, 2), 1e-10, 1000, iters, relres);
    c.putSolve("esc.solve", ok, iters, relres, nullptr, nullptr);

    // the coarse branch on the operator of the eigensolver case: vectors from outside, then its own
    // (the constructor names the transfer for the reader and never looks at it)
    Eigsolve_Mugiq esE(head(start, 3), HT0, Eop, Hg, nullptr, EopIn.kappa);
    esE.computeEvals();
    putEvals(c, "ese.given", *esE.getEvals(), *esE.getEvalsRes(), *esE.getEvalsSigma());
    CoarseEigParam ep;
    ep.nConv = nConv; ep.nKr = nKr; ep.polyDeg = 20; ep.tol = 1e-10;
    const MugiqHipCoarseEigInfo info = esE.computeEvecs(c.newC("ese.ev.", nConv, EopIn.X, EopIn.nVec), start, ep);
    putEigInfo(c, "ese.info", info);
    c.putI("ese.nCoarseEvecs", (long long)esE.getCoarseEvecs().size());
    c.putZ("ese.quda", *esE.getEvalsQuda());
    c.putI("ese.sigmaAfterEvecs", (long long)esE.getEvalsSigma()->size());
    esE.computeEvals();
    putEvals(c, "ese.own", *esE.getEvals(), *esE.getEvalsRes(), *esE.getEvalsSigma());
    c.putS("ese.print", printed(esE, c.dir + "/print.coarse.txt"));
  }

  // host queries
  {
    const MugiqHipFusedForm f = fusedForm(r[0], 2, {1, 2});
    c.putI("fusedForm", std::vector<long long>{f.kernel, f.family, f.slotsPerLaunch, f.packCapacity, f.gaugeBytes, f.nSlots, f.kmax, f.waves, f.staged, f.tj,
                                               f.lines, f.rowGroups, f.rows, f.rowChunk, f.leftBufElems, f.ph, f.glds, f.npc, f.np, f.m, f.phl, f.ldsBytes});
    const MugiqHipTransferForm t = transferForm(HT0, 4);
    c.putI("transferForm", std::vector<long long>{t.X[0], t.X[1], t.X[2], t.X[3], t.Xc[0], t.Xc[1], t.Xc[2], t.Xc[3], t.bs[0], t.bs[1], t.bs[2], t.bs[3], t.aggVol,
                                                  t.volumeCB, t.volumeCBc, t.coarseNColor, t.coarseStride, t.coarseParityOffset, t.prolongFamily, t.prolongThreads,
                                                  t.prolongWorkgroups, t.prolongPasses, t.prolongBlocksPerPass, t.prolongLdsBytes, t.prolongWorkspaceBytes,
                                                  t.contractFamily, t.contractThreads, t.contractWorkgroups, t.JC, t.SPR, t.NH, t.outerB, t.glds,
                                                  t.contractLdsBytes, t.contractScratchBytes});
  }

  // the loop level, where tests/cpp/loop.cpp does not go: the gamma tables, the batched contraction, the three stages of the momentum
  // projection, computeLoop, a loop object's device data, entry kernel and deflation (fine and coarse), Displace's state and auxiliary vector
  {
    copyGammaCoeffStructToSymbol<double>();
    copyGammaMapStructToSymbol<double>();
    std::string gammas;
    for (int m = 0; m < 16; m++) gammas += GammaName(m) + "\n";
    c.putS("lp.gammaNames", gammas);
    bool threw = false;
    try {
      GammaName(16);
    } catch (const std::out_of_range &) {
      threw = true;
    }
    c.putI("lp.gammaName16Throws", threw ? 1 : 0);

    const int V = Hg.X[0] * Hg.X[1] * Hg.X[2] * Hg.X[3], locT = Hg.X[3], nData = 16, Nmom = 3;
    const long long locV3 = V / locT;
    const std::vector<double> lsig = {0.5, 1.0, 2.0, 4.0};
    auto download = [&](const std::string &name, const void *d, size_t n) {
      std::vector<cplx> h(n);
      HIPX(hipMemcpy(h.data(), d, n * sizeof(cplx), hipMemcpyDeviceToHost));
      c.putZ(name, h);
    };
    cplx *loop_d = nullptr, *phase_d = nullptr, *mp_d = nullptr, *mom_d = nullptr;
    HIPX(hipMalloc(&loop_d, (size_t)nData * V * sizeof(cplx)));
    HIPX(hipMemset(loop_d, 0, (size_t)nData * V * sizeof(cplx)));
    HIPX(hipMalloc(&phase_d, (size_t)locV3 * Nmom * sizeof(cplx)));
    HIPX(hipMalloc(&mp_d, (size_t)nData * V * sizeof(cplx)));
    HIPX(hipMalloc(&mom_d, (size_t)locT * nData * Nmom * sizeof(cplx)));
    performLoopContractionBatched<double, FLOAT4_FIELD_ORDER>(loop_d, ev, ev, lsig);
    download("lp.loop", loop_d, (size_t)nData * V);
    const std::vector<double> &momD = c.S("lp.mom");
    const std::vector<int> mom(momD.begin(), momD.end());
    createPhaseMatrixGPU<double>(phase_d, mom.data(), locV3, Nmom, (int)LOOP_FT_SIGN_PLUS, Hg.X, Hg.X);
    download("lp.phase", phase_d, (size_t)locV3 * Nmom);
    convertIdxOrder_mapGamma<double>(mp_d, loop_d, nData, 1, 2, V / 2, Hg.X);
    download("lp.posMP", mp_d, (size_t)nData * V);
    momentumProjectionGemm<double>(mom_d, mp_d, phase_d, locT, nData, locV3, Nmom);
    download("lp.dataMom", mom_d, (size_t)locT * nData * Nmom);

    MugiqLoopParam plain;
    computeLoop<double, FLOAT4_FIELD_ORDER>(plain, ev, lsig);  // ultra-local, nothing to write: the warning of the reference
    MugiqLoopParam lp;
    setDisplaceEntryString(lp, "+z:1");
    lp.gauge_ext = &Hg;
    {
      Loop_Mugiq<double, FLOAT4_FIELD_ORDER> loop(&lp, ev, sigmaH);
      loop.computeCoarseLoop();
      const MugiqHipLoopInfo info = loop.info();
      c.putI("lp.nLoop", info.nLoop);
      c.putI("lp.entryKernel", std::vector<int>{loop.entryKernel(0), loop.entryKernel(1)});
      const size_t n = (size_t)info.nLoop * nData * V;
      download("lp.dataPos_d", loop.dataPos_d(), n);
      std::vector<cplx> h(n);
      HIPX(hipMemcpy(h.data(), loop.dataPos_d(), n * sizeof(cplx), hipMemcpyDeviceToHost));
      c.putI("lp.dataPosEqualsDevice", memcmp(h.data(), loop.dataPos(), n * sizeof(cplx)) == 0 ? 1 : 0);
      std::vector<cplx> overlaps;
      loop.deflate(c.copyF("lp.dl.", "r", 6, 2), c.Fs("r", 4, 2), true, &overlaps);  // == deflateLowModes(..., ev, sigmaH, true, &overlaps)
      c.putZ("lp.dl.overlaps", overlaps);
    }
    {
      MugiqLoopParam none;
      Loop_Mugiq<double, FLOAT2_FIELD_ORDER> coarse(&none, head(w, 3), c.S("dlc.sigma"), {HT0, HT1});
      coarse.deflateCoarse(c.copyF("lp.dlc.", "r", 6, 2), c.Fs("r", 4, 2), false);  // == deflateLowModesCoarse(..., {HT0, HT1}, sigma, false)
    }
    {
      ColorSpinorField r0 = r[0], out = c.newF("lp.aux.", 1, "r0")[0];
      Displace<double, FLOAT4_FIELD_ORDER> displace(&lp, &r0, 8);
      displace.setupDisplacement("+z");
      c.putI("lp.displace", std::vector<int>{(int)displace.dir(), (int)displace.sign(), displace.gauge() == &Hg ? 1 : 0});
      c.putI("lp.which", std::vector<int>{(int)displace.WhichDisplaceFlag(), (int)displace.WhichDisplaceDir(), (int)displace.WhichDisplaceSign()});
      displace.resetAuxDispVec(&r0);
      displace.swapAuxDispVec(&out);
      // one covariant step along +z, through the state machine and through the wrapper it calls
      ColorSpinorField moved = c.copyF("lp.moved.", "r", 0, 1)[0], direct = c.newF("lp.direct.", 1, "r0")[0];
      displace.doVectorDisplacement(DISPLACE_TYPE_COVARIANT, &moved, 1);
      GaugeField g = Hg;
      exchangeGhostVec(&r0);
      performCovariantDisplacementVector<double, FLOAT4_FIELD_ORDER>(&direct, &r0, &g, DispDir_z, DispSignPlus);
    }
    HIPX(hipDeviceSynchronize());
    HIPX(hipFree(loop_d));
    HIPX(hipFree(phase_d));
    HIPX(hipFree(mp_d));
    HIPX(hipFree(mom_d));
  }

  // errors: a size mismatch the wrapper refuses and a call the library refuses, per family; nothing here reaches a kernel
  {
    std::vector<cplx> lam;
    std::vector<double> res, sig;
    const std::vector<ColorSpinorField> one = head(r, 1), two = head(r, 2);
    c.expectError("err.deflate.size", [&] { deflateLowModes(one, two, ev); });
    c.expectError("err.deflate.lib", [&] { deflateLowModes(head(r32, 2), two, ev); });
    c.expectError("err.restrict.size", [&] { restrictVecs(head(rc, 1), two, HT0); });
    c.expectError("err.restrict.lib", [&] { restrictVecs(head(w, 2), two, HT0); });
    c.expectError("err.wilson.size", [&] { wilsonApply(one, two, Hg, kappa); });
    c.expectError("err.wilson.lib", [&] { wilsonApply(two, two, Hg, kappa, 17); });
    c.expectError("err.evals.size", [&] { computeEvals({}, Hg, kappa, M, false, lam, res, sig); });
    c.expectError("err.solve.size", [&] { wilsonSolve(two, two, Hg, kappa, ev, {}, 1e-10, 10, iters, relres); });
    c.expectError("err.solve.lib", [&] { wilsonSolve(two, two, Hg, kappa, {}, {}, -1.0, 10, iters, relres); });
    c.expectError("err.coarseop.lib", [&] { computeCoarseOperator(op1s, HT0, Hg, &Hcl, kappa); });  // operator precision != transfer precision
    c.expectError("err.getCoarseVector.lib", [&] { getCoarseVector(rc[0], HT1, HT1.nVec); });
    c.expectError("err.coarseApply.size", [&] { coarseApply(head(w, 1), head(w, 2), op2); });
    c.expectError("err.coarseApply.lib", [&] { coarseApply(head(rc, 2), head(w, 2), op2); });
    c.expectError("err.coarseApplyForm.lib", [&] { coarseApplyForm(*op2.desc(), 0); });
    c.expectError("err.mg.size", [&] { mgPrecondition(two, two, Hg, &Hcl, kappa, std::vector<MugiqHipTransfer>{HT0, HT1}, {*op1.desc()}, {MgSolveParam()}); });
    c.expectError("err.mg.lib", [&] { mgPrecondition(two, two, Hg, &Hcl, kappa, HT0, op1s); });
    c.expectError("err.mgSolve.lib", [&] { mgSolve(two, two, Hg, &Hcl, kappa, HT0, op1, solveParam(17, 0, 4, 4), iters, relres); });
    c.expectError("err.setup.size", [&] { mgSetup(HT0, nullptr, {}, Hg, &Hcl, kappa); });
    c.expectError("err.gram.size", [&] { coarseGram({}, w); });
    c.expectError("err.gram.lib", [&] { coarseGram(head(w, 2), head(rc, 2)); });
    c.expectError("err.rotate.size", [&] { coarseRotate(head(w, 2), head(w, 3), std::vector<cplx>(5)); });
    c.expectError("err.eig.size", [&] { CoarseEigParam ep; coarseEigensolve(head(w, 2), head(w, 3), op2, MDAGM, ep, res, res, sig); });
    c.expectError("err.smear.lib", [&] { stoutSmear(Hg, Hg, 0.1, 1); });  // out overlaps in
    c.expectError("err.cholesky.lib", [&] { std::vector<cplx> R; choleskyUpper(2, std::vector<cplx>{1.0, 1.0, 1.0, 1.0}, R); });
  }
}

// ---- --host-selftest -----------------------------------------------------------------------------------------------------------------
#define EXPECT(cond)                                                            \
  do {                                                                          \
    if (!(cond)) {                                                              \
      fprintf(stderr, "host selftest failed at line %d: %s\n", __LINE__, #cond); \
      return 1;                                                                 \
    }                                                                           \
  } while (0)

static int hostSelftest(int argc, char **argv) {
  std::vector<int> iters;
  std::vector<double> relres;
  int stride = -1;
  // mgOutputs
  std::vector<double> hist = detail::mgOutputs(3, 0, true, iters, relres, &stride);
  EXPECT(stride == 1 && hist.size() == 3 && iters.size() == 3 && relres.size() == 3);
  hist = detail::mgOutputs(3, 7, false, iters, relres, &stride);
  EXPECT(stride == 7 && hist.empty() && iters == std::vector<int>(3, 0) && relres == std::vector<double>(3, 0.0));
  hist = detail::mgOutputs(3, 7, true, iters, relres, &stride);
  EXPECT(stride == 7 && hist.size() == 21);
  // mgHistory: right-hand side i wrote 100 i + k at i * stride + k
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 7; k++) hist[i * 7 + k] = 100.0 * i + k;
  iters = {2, 0, 5};
  std::vector<std::vector<double>> history(9);
  EXPECT(detail::mgHistory(0, hist, 7, iters, &history));
  EXPECT(history.size() == 3 && history[0] == (std::vector<double>{0.0, 1.0}) && history[1].empty() &&
         history[2] == (std::vector<double>{200.0, 201.0, 202.0, 203.0, 204.0}));
  history.clear();
  EXPECT(!detail::mgHistory(MUGIQ_HIP_ERROR_NOT_CONVERGED, hist, 7, iters, &history));
  EXPECT(history.size() == 3 && history[2].size() == 5 && history[2][4] == 204.0);
  EXPECT(detail::mgHistory(0, hist, 7, iters, nullptr));
  EXPECT(!detail::mgHistory(MUGIQ_HIP_ERROR_NOT_CONVERGED, std::vector<double>(), 7, iters, nullptr));
  bool threw = false;
  try {
    detail::mgHistory(MUGIQ_HIP_ERROR_INVALID_ARGUMENT, hist, 7, iters, &history);
  } catch (const Error &e) {
    threw = e.status == 1;
  }
  EXPECT(threw);
  // mgLevels
  const std::vector<MugiqHipTransfer> t2(2);
  const std::vector<MugiqHipCoarseOperator> o2(2), o1(1);
  const MugiqHipMgSolveParam raw = {1e-10, 1000, 16, 0, 4, 1.0, 8};
  std::vector<MgSolveParam> p2;
  EXPECT(sizeof(MgSolveParam) == sizeof(MugiqHipMgSolveParam));
  for (int bad = 0; bad < 3; bad++) {
    threw = false;
    try {
      if (bad == 0) detail::mgLevels(t2, o1, p2, "selftest");
      else if (bad == 1) detail::mgLevels(t2, o2, p2, "selftest");
      else detail::mgLevels({}, {}, {}, "selftest");
    } catch (const Error &e) {
      threw = e.status == 1 && std::string(e.what()).find("selftest: one transfer") == 0;
    }
    EXPECT(threw);
  }
  (void)raw;
  // the dense helpers on the 5 x 5 matrices passed in: H, G (row-major complex as %a pairs), then theta, |Z| is not unique, so what is
  // checked against the values passed in is theta, R and R^-1; Z through H Z = Z diag(theta)
  if (argc < 3) return 0;
  std::vector<double> v;
  {
    std::ifstream f(argv[2]);
    std::string tok;
    while (f >> tok) v.push_back(strtod(tok.c_str(), nullptr));
  }
  const int n = 5, nn = 25;
  EXPECT(v.size() == (size_t)(2 * nn + 2 * nn + n + 2 * nn + 2 * nn));
  auto zs = [&](size_t off, int count) {
    std::vector<cplx> z(count);
    for (int i = 0; i < count; i++) z[i] = cplx(v[off + 2 * i], v[off + 2 * i + 1]);
    return z;
  };
  const std::vector<cplx> Hm = zs(0, nn), Gm = zs(50, nn), wantR = zs(105, nn), wantRinv = zs(155, nn);
  std::vector<double> theta;
  std::vector<cplx> Z, R, Rinv;
  hermitianEigh(n, Hm, theta, Z);
  double scale = 0.0;
  for (const cplx &h : Hm) scale = std::max(scale, std::abs(h));
  for (int i = 0; i < n; i++) EXPECT(std::abs(theta[i] - v[100 + i]) <= 1e-13 * scale);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) {
      cplx hz = 0.0, zz = 0.0;
      for (int k = 0; k < n; k++) {
        hz += Hm[i * n + k] * Z[k * n + j];
        zz += std::conj(Z[k * n + i]) * Z[k * n + j];
      }
      EXPECT(std::abs(hz - Z[i * n + j] * theta[j]) <= 1e-13 * scale);
      EXPECT(std::abs(zz - (i == j ? 1.0 : 0.0)) <= 1e-13);
    }
  choleskyUpper(n, Gm, R);
  upperTriangularInverse(n, R, Rinv);
  double rs = 0.0, ris = 0.0;
  for (int i = 0; i < nn; i++) {
    rs = std::max(rs, std::abs(wantR[i]));
    ris = std::max(ris, std::abs(wantRinv[i]));
  }
  for (int i = 0; i < nn; i++) {
    EXPECT(std::abs(R[i] - wantR[i]) <= 1e-13 * rs);
    EXPECT(std::abs(Rinv[i] - wantRinv[i]) <= 1e-12 * ris);
  }
  // rank-deficient G = u u^dag: status 1
  std::vector<cplx> G1(nn);
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++) G1[i * n + j] = cplx(i + 1.0, 0.5) * std::conj(cplx(j + 1.0, 0.5));
  threw = false;
  try {
    choleskyUpper(n, G1, R, 1e-8);
  } catch (const Error &e) {
    threw = e.status == 1;
  }
  EXPECT(threw);
  return 0;
}

int main(int argc, char **argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "--list") {
    for (const char *n : EXECUTED) printf("%s\n", n);
    return 0;
  }
  if (mode == "--host-selftest") {
    try {
      const int rc = hostSelftest(argc, argv);
      printf(rc == 0 ? "HOST SELFTEST PASSED\n" : "HOST SELFTEST FAILED\n");
      return rc;
    } catch (const std::exception &e) {
      die(4, std::string("unexpected exception: ") + e.what());
    }
  }
  if (mode == "--parse-only" && argc > 2) {
    const std::string dir = argv[2];
    std::ofstream f(dir + "/manifest.out.txt");
    for (const Obj &o : readManifest(dir)) f << formatLine(o) << "\n";
    return f.good() ? 0 : 2;
  }
  if (mode.empty() || mode[0] == '-') {
    fprintf(stderr, "usage: operators_cpp_test DIR | --list | --host-selftest [FILE] | --parse-only DIR\n");
    return 2;
  }
  Case c;
  c.dir = mode;
  c.res = fopen((c.dir + "/results.txt").c_str(), "w");
  if (!c.res) die(2, "cannot write " + c.dir + "/results.txt");
  try {
    c.load();
    run(c);
    c.writeOutputs();
  } catch (const Error &e) {
    die(4, "unexpected mugiq_hip::Error " + std::to_string(e.status) + ": " + e.what());
  } catch (const std::exception &e) {
    die(4, std::string("unexpected exception: ") + e.what());
  }
  fclose(c.res);
  printf("OPERATORS TEST RAN\n");
  fflush(nullptr);
  _Exit(0);  // the buffers go with the process
}
