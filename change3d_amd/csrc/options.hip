// The library-wide runtime switches (c3d_set_option; what each one means is documented at the C3D_OPT_* ids in
// include/change3d_hip.h) and c3d_last_kernel.  Every option variable is defined HERE, once, from the table below; the
// translation units that read one see it through launch_hints.h.
#include "../../include/change3d_hip.h"
#include "common.h"
#include "launch_hints.h"
#include <cstring>
#include <cxxabi.h>

namespace {
// how c3d_set_option turns the caller's value into the stored one
enum Norm {
  BOOL,     // value ? 1 : 0
  CLAMP,    // clamped to 0 .. arg
  MASK,     // value & arg
  BIT_OFF,  // (value & arg) ? 0 : 1
};
}  // namespace

// One row per option variable: id, variable, normalisation, its argument, default.
// C3D_OPT_PW_WGRAD_V2 has two rows: bit 0 selects the kernel, bit 1 CLEAR = chained reduction of the separate weight gradients.
#define C3D_OPTIONS(X)                                                    \
  X(C3D_OPT_SIDE_STREAM, c3d_option_side_stream, BOOL, 0, 1)              \
  X(C3D_OPT_STEM_MFMA, c3d_option_stem_mfma, CLAMP, 2, 2)                 \
  X(C3D_OPT_CONVT_MFMA, c3d_option_convt_mfma, BOOL, 0, 1)                \
  X(C3D_OPT_FUSE_WGRAD, c3d_option_fuse_wgrad, MASK, 3, 3)                \
  X(C3D_OPT_FOLD_SE, c3d_option_fold_se, BOOL, 0, 1)                      \
  X(C3D_OPT_MASK_IN_DGRAD, c3d_option_mask_in_dgrad, MASK, 3, 3)          \
  X(C3D_OPT_DW_RING, c3d_option_dw_ring, MASK, 15, 13)                    \
  X(C3D_OPT_PW_WGRAD_V2, c3d_option_pw_wgrad_v2, MASK, 1, 1)              \
  X(C3D_OPT_PW_WGRAD_V2, c3d_option_wgrad_chain, BIT_OFF, 2, 1)           \
  X(C3D_OPT_DW_FWD_HV, c3d_option_dw_fwd_hv, MASK, 7, 5)                  \
  X(C3D_OPT_PW_CFWD, c3d_option_pw_cfwd, MASK, 3, 3)                      \
  X(C3D_OPT_PW_CDG, c3d_option_pw_cdg, MASK, 3, 3)                        \
  X(C3D_OPT_DW_T4, c3d_option_dw_t4, BOOL, 0, 1)

#define X(id, var, how, arg, dflt) int var = dflt;
C3D_OPTIONS(X)
#undef X

extern "C" int c3d_set_option(int32_t option, int32_t value) {
  static const struct { int32_t id; int* var; Norm how; int arg; } rows[] = {
#define X(id, var, how, arg, dflt) {id, &var, how, arg},
      C3D_OPTIONS(X)
#undef X
  };
  int rc = C3D_E_BADARG;
  for (const auto& r : rows) {
    if (r.id != option) continue;
    switch (r.how) {
      case BOOL: *r.var = value ? 1 : 0; break;
      case CLAMP: *r.var = value < 0 ? 0 : (value > r.arg ? r.arg : value); break;
      case MASK: *r.var = value & r.arg; break;
      case BIT_OFF: *r.var = (value & r.arg) ? 0 : 1; break;
    }
    rc = 0;
  }
  return rc;
}

extern "C" int64_t c3d_launch_count(void) { return c3d_launches; }

// The runtime knows the mangled device name of every registered kernel by its host handle; demangled, that is
// "void (anonymous namespace)::dw_fwd_v2_kernel<unsigned short, 3, true, true>(unsigned short const*, ...)" (bf16_t is unsigned
// short): return type, namespace and parameter list are cut, the template arguments stay.
extern "C" const char* c3d_last_kernel(void) {
  static thread_local char name[256];
  name[0] = 0;
  if (!c3d_last_launch) return name;
  const char* mangled = hipKernelNameRefByPtr(c3d_last_launch, nullptr);
  if (!mangled) return name;
  int status = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  const char* s = d ? d : mangled;
  if (!strncmp(s, "void ", 5)) s += 5;
  static const char anon[] = "(anonymous namespace)::";
  size_t o = 0;
  for (int depth = 0; *s && o + 1 < sizeof(name);) {
    if (!strncmp(s, anon, sizeof(anon) - 1)) { s += sizeof(anon) - 1; continue; }
    if (*s == '(' && depth == 0) break;   // the parameter list
    depth += (*s == '<') - (*s == '>');
    name[o++] = *s++;
  }
  name[o] = 0;
  free(d);
  return name;
}
