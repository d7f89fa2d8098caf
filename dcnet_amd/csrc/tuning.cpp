// The registry behind tuning.h: dcn_set_tuning (exact names) and dcn_tuning_info (enumeration).
#include "common.h"
#include "tuning.h"
#include <string.h>

static DcnKnob* g_knobs = nullptr;      // sorted by name; zero-initialised before any knob's constructor runs

DcnKnob::DcnKnob(const char* name_, int* var_, int def_, const char* desc_, int (*norm_)(int), const char* abl_flag_, bool abl_on_,
                 bool (*abl_value_)(int))
    : name(name_), var(var_), def(def_), desc(desc_), norm(norm_), abl_flag(abl_flag_), abl_on(abl_on_), abl_value(abl_value_) {
  DcnKnob** at = &g_knobs;
  while (*at && strcmp((*at)->name, name) < 0) at = &(*at)->next;
  next = *at;
  *at = this;
}

extern "C" int dcn_set_tuning(const char* key, int value) {
  DCN_CHECK_ARG(key, "set_tuning: null key");
  for (DcnKnob* k = g_knobs; k; k = k->next) {
    if (strcmp(k->name, key) != 0) continue;
    DCN_CHECK_ARG(!k->abl_flag || k->abl_on || !(k->abl_value ? k->abl_value(value) : value != 0),
                  "set_tuning: \"%s\" = %d makes results wrong by construction and exists only in builds with %s", key, value, k->abl_flag);
    *k->var = k->norm ? k->norm(value) : value;
    return DCN_OK;
  }
  dcn_set_error("set_tuning: unknown key \"%s\" (names are matched exactly; dcn_tuning_info lists them)", key);
  return DCN_ERR_ARG;
}

extern "C" int dcn_tuning_info(int index, const char** name, int* value, int* def, const char** desc, int* ablation) {
  DcnKnob* k = g_knobs;
  for (int i = 0; k && i < index; ++i) k = k->next;
  DCN_CHECK_ARG(index >= 0 && k, "tuning_info: index %d is past the last knob", index);
  if (name) *name = k->name;
  if (value) *value = *k->var;
  if (def) *def = k->def;
  if (desc) *desc = k->desc;
  if (ablation) *ablation = (k->abl_flag && !k->abl_value) ? (k->abl_on ? 2 : 1) : 0;
  return DCN_OK;
}
