// Experiment knobs of libdcnet_hip.so: ONE declaration per knob, next to the code that reads it.
//
//   DCN_KNOB(g_conv3, "3x3strip", 1, "conv3.hip: 3x3 stride-1 layers on the strip kernel (0 = implicit-GEMM tile)");
//
// defines the plain `int g_conv3 = 1` the launch code reads and registers it under its exact name for dcn_set_tuning /
// dcn_tuning_info (tuning.cpp).  Optional further arguments, in this order:
//   norm      int (*)(int): what the setter stores for a requested value (nullptr = the value itself)
//   abl_flag  the compile flag without which some values of the knob are refused: they make results wrong by construction
//   abl_on    whether this build was compiled with that flag
//   abl_value bool (*)(int): which values those are (nullptr = every non-zero value: the knob exists only in ablation builds)
#pragma once

// -DDCN_ABL=1 (DCN_EXTRA_FLAGS): compiles the timing-only ablations of igemm.hip / wgrad.hip ("abl") and the slab pass that
// writes nothing ("Slabfold" < 0) in.  Results are WRONG with them; a default build has neither the code nor the switch.
#ifndef DCN_ABL
#define DCN_ABL 0
#endif

struct DcnKnob {
  const char* name; int* var; int def; const char* desc;
  int (*norm)(int);
  const char* abl_flag; bool abl_on; bool (*abl_value)(int);
  DcnKnob* next;
  DcnKnob(const char* name, int* var, int def, const char* desc, int (*norm)(int) = nullptr,
          const char* abl_flag = nullptr, bool abl_on = false, bool (*abl_value)(int) = nullptr);
};

#define DCN_KNOB(var, name, def, ...) int var = def; static DcnKnob knob_##var(name, &var, def, __VA_ARGS__)
