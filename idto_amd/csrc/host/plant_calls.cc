// plant_calls.cc — see plant_calls.h.  The messages and the order of the checks within an entry are contract: the first refusal
// wins, and callers match the text.
#include "host/plant_calls.h"

#include <algorithm>
#include <cmath>

#include "plant_sizes.h"
#include "plant_tangent.h"

namespace idto_host {

using idto_plant::lin_columns;

// ---- block and LDS

size_t PlantPdDoubles(const PlantShape& s) { return idto_dev::plant_pd_doubles(s.nq, s.nv, s.mpc_nu, s.mpc_n, s.mpc_len); }

int PlantLdsBytes(const PlantShape& s, int threads, size_t beside) {
  const size_t d = (size_t)idto_dev::plant_lds_doubles(s.nq, s.nv, s.blob_n, s.nxb, s.nstem, s.npaths, threads) + beside;
  return d > (size_t)1 << 24 ? 1 << 27 : (int)(d * sizeof(double));
}

int PlantBlock(const PlantShape& s, int forced, size_t beside) {
  int t = forced ? forced : std::min(256, (((s.nv + 1) * s.npaths + 63) / 64) * 64);
  while (t > 64 && PlantLdsBytes(s, t, beside) > kPlantMaxLds) t -= 64;
  return t;
}

// ---- layouts

namespace {

struct Carver {
  CallPlan p;
  size_t at = 0, end = 0;
  void Take(const char* name, size_t count) { p.entries.push_back({name, at, count}); at += (count + 7) / 8 * 8; }
  void MirrorOnly(const char* name, size_t offset, size_t count) { p.entries.push_back({name, offset, count}); end = offset + count; }
  // the device buffer ends behind the last entry carved; the mirror holds the inputs, then what lies from out0 to a mirror-only
  // entry's end, or to the buffer's
  CallPlan Done() {
    p.total = at;
    p.pinned = std::max(p.in_n, (end ? end : at) - p.out0);
    return p;
  }
};
#define IDTO_PLAN_TAKE(name, count) k.Take(#name, count);
#define IDTO_PLAN_IN k.p.in_n = k.at;
#define IDTO_PLAN_OUT k.p.out0 = k.at;

}  // namespace

CallPlan PlanPlantStorage(const PlantShape& s, size_t rec_n, int record_capacity, int nu_) {
  const size_t B = (size_t)s.batch, nq = (size_t)s.nq, nv = (size_t)s.nv, w = nq + nv, cap = (size_t)PlantRecordCapacity(record_capacity), nu = (size_t)nu_;
  Carver k;
  IDTO_PLANT_STORAGE_PLAN(IDTO_PLAN_TAKE, IDTO_PLAN_IN, IDTO_PLAN_OUT)
  k.p.in_n = B * (w + nv);
  k.MirrorOnly("status_back", k.p.at(plant_storage::fd_bias) + B * nv, B);   // (right behind the bias, not on a boundary)
  return k.Done();
}

CallPlan PlanScene(const PlantShape& s, int nstates, unsigned mask) {
  const size_t B = (size_t)s.batch, S = (size_t)nstates, nb = (size_t)s.nb, np = (size_t)s.npairs, nv = (size_t)s.nv;
  Carver k;
  IDTO_SCENE_PLAN(IDTO_PLAN_TAKE, IDTO_PLAN_IN, IDTO_PLAN_OUT)
  k.p.in_n = B * S * (size_t)(s.nq + s.nv);
  CallPlan p = k.Done();
  p.pinned = std::max<size_t>(p.pinned, 8);   // (the outputs' buffer is never empty)
  return p;
}

CallPlan PlanLin(const PlantShape& s, int nstates, bool tv, int nu_) {
  const size_t B = (size_t)s.batch, S = (size_t)nstates, nv = (size_t)s.nv, w = (size_t)(s.nq + s.nv), n = 2 * nv, nu = tv ? (size_t)nu_ : 0,
               SP = S * (size_t)lin_columns(s.nv);
  Carver k;
  IDTO_LIN_PLAN(IDTO_PLAN_TAKE, IDTO_PLAN_IN, IDTO_PLAN_OUT)
  return k.Done();
}

CallPlan PlanTrack(const PlantShape& s, int nsteps, int nrollouts, int nu_, bool own_K) {
  const size_t B = (size_t)s.batch, S = (size_t)nsteps, R = (size_t)nrollouts, nv = (size_t)s.nv, w = (size_t)(s.nq + s.nv), n = 2 * nv, nu = (size_t)nu_;
  Carver k;
  IDTO_TRACK_PLAN(IDTO_PLAN_TAKE, IDTO_PLAN_IN, IDTO_PLAN_OUT)
  k.MirrorOnly("status_back", k.at, B * R);
  return k.Done();
}

// ---- refusals

namespace {

#define REFUSE_IF(cond, text) do { if (cond) return Refusal{-1, std::string(who) + ": " + (text)}; } while (0)
#define PASS(check) do { if (Refusal r_ = (check); r_.rc) return r_; } while (0)

Refusal Substeps(const char* who, int substeps) {
  REFUSE_IF(substeps < 1 || substeps > IDTO_PLANT_MAX_SUBSTEPS, "substeps must be in [1, 4096] (a single launch stays short on a shared device)");
  return {};
}
Refusal StepH(const char* who, double h) {
  REFUSE_IF(!(h > 0.0) || !std::isfinite(h), "the substep h must be > 0 and finite");
  return {};
}
Refusal Models(const PlantShape& s, const char* who, int models) {
  REFUSE_IF(models != IDTO_SCENE_MODELS_PROBLEMS && models != IDTO_SCENE_MODELS_PLANTS, "models is IDTO_SCENE_MODELS_PROBLEMS or IDTO_SCENE_MODELS_PLANTS");
  REFUSE_IF(models == IDTO_SCENE_MODELS_PLANTS && !s.plants_begun, "the plants' models were asked for: call idto_hip_plant_begin on the context first");
  return {};
}
Refusal NoChildren(const PlantShape& s, const char* who) {
  REFUSE_IF(s.children, "this context has child contexts (the child-context route of idto_hip_tr_solve_batch_constrained made them)");
  return {};
}
// the classes of model that plant_kernel serves
Refusal Serves(const PlantShape& s, const char* who) {
  REFUSE_IF(s.nv > 64, "nv > 64 (the solve of M a = tau - c runs a lane per row on one wavefront)");
  return {};
}
Refusal NuRange(const PlantShape& s, const char* who, int nu) {
  REFUSE_IF(nu < 1 || nu > s.nv, "nu must be in [1, nv]");
  return {};
}
Refusal Actuated(const PlantShape& s, const char* who, int nu, const int* actuated) {
  for (int i = 0; i < nu; ++i)
    REFUSE_IF(actuated[i] < 0 || actuated[i] >= s.nv, "actuated[" + std::to_string(i) + "] is not a velocity index in [0, nv)");
  return {};
}
Refusal Finite(const char* who, const char* what, const double* p, size_t count) {
  for (size_t i = 0; i < count; ++i) REFUSE_IF(!std::isfinite(p[i]), std::string(what) + " is not finite at index " + std::to_string(i));
  return {};
}

}  // namespace

Refusal RefusePlantsBegun(const PlantShape& s, const char* who) {
  REFUSE_IF(!s.plants_begun, "call idto_hip_plant_begin on the context first");
  return {};
}

Refusal RefusePlantBegin(const PlantShape& s, const idto_plant_params_t* prm) {
  const char* who = "plant_begin";
  REFUSE_IF(!prm, "parameters are required");
  PASS(NoChildren(s, who));
  REFUSE_IF(!(prm->h > 0.0) || !std::isfinite(prm->h), "the substep h must be > 0");
  REFUSE_IF(prm->mode != IDTO_PLANT_HOLD && prm->mode != IDTO_PLANT_PD_PLUS, "mode is IDTO_PLANT_HOLD or IDTO_PLANT_PD_PLUS");
  PASS(Serves(s, who));
  REFUSE_IF(prm->block_threads != 0 && (prm->block_threads % 64 != 0 || prm->block_threads < 64 || prm->block_threads > 256),
            "block_threads is 0, 64, 128, 192 or 256");
  REFUSE_IF(prm->record_capacity < 0, "record_capacity must not be negative");
  if (prm->mode == IDTO_PLANT_PD_PLUS) {
    REFUSE_IF(!s.mpc, "PD+ needs the stored plans: call idto_hip_mpc_batch_begin (and idto_hip_mpc_batch_store) on the context first");
    const int nu = s.mpc_nu;
    REFUSE_IF(!prm->Kp || !prm->Kd || prm->kp_size != nu * s.nq || prm->kd_size != nu * s.nv,
              "gains of the wrong size: Kp is [nu][nq] = " + std::to_string(nu * s.nq) + " and Kd [nu][nv] = " + std::to_string(nu * s.nv) + " doubles");
    for (int i = 0; i < prm->kp_size; ++i) REFUSE_IF(!std::isfinite(prm->Kp[i]), "a gain in Kp is not finite");
    for (int i = 0; i < prm->kd_size; ++i) REFUSE_IF(!std::isfinite(prm->Kd[i]), "a gain in Kd is not finite");
  }
  return {};   // (then RefusePlantStorage, where the storage is made)
}

Refusal RefusePlantStorage(const PlantShape& s, int block_threads, bool pd) {
  const char* who = "plant_begin";
  REFUSE_IF(!s.host_model, "the context keeps no host copy of its model");
  const size_t beside = pd ? PlantPdDoubles(s) : 0;
  REFUSE_IF(PlantLdsBytes(s, PlantBlock(s, block_threads, beside), beside) > kPlantMaxLds,
            "the model, a substep's evaluations and the plan do not fit the 160 KiB of LDS");
  return {};
}

Refusal RefusePlantSetModel(const PlantShape& s, int b) {
  const char* who = "plant_set_model";
  PASS(RefusePlantsBegun(s, who));
  REFUSE_IF(b < 0 || b >= s.batch, "plant index outside the batch");
  return {};
}

Refusal RefusePlantSetState(const PlantShape& s, const double* times, const double* x) {
  const char* who = "plant_set_state";
  PASS(RefusePlantsBegun(s, who));
  REFUSE_IF(!times || !x, "times[batch] and x[batch][nq + nv] are required");
  return {};
}

Refusal RefusePlantStep(const PlantShape& s, const char* who, int substeps, const double* tau_hold, int record_every, bool record, int* nrec) {
  PASS(RefusePlantsBegun(s, who));
  PASS(Substeps(who, substeps));
  const bool pd = s.plant_mode == IDTO_PLANT_PD_PLUS;
  REFUSE_IF(!pd && !tau_hold, "hold mode needs tau_hold[batch][nv]");
  REFUSE_IF(pd && tau_hold, "PD+ forms the torque itself: tau_hold must be NULL");
  // (the plans the LDS was sized for at idto_hip_plant_begin: the same idto_hip_mpc_batch_begin, not only the same sizes)
  REFUSE_IF(pd && (!s.mpc || !s.plant_mpc_current || s.mpc_nu != s.plant_nu || PlantLdsBytes(s, s.plant_block, PlantPdDoubles(s)) != s.plant_lds),
            "PD+: idto_hip_mpc_batch_begin was called again after idto_hip_plant_begin (call idto_hip_plant_begin again)");
  *nrec = 0;
  if (record) {
    REFUSE_IF(record_every < 1, "record_every must be >= 1 with x_record_out");
    *nrec = substeps / record_every;
    REFUSE_IF(*nrec > s.plant_record_capacity, "more recorded states than idto_hip_plant_begin's record_capacity");
  }
  return {};
}

Refusal RefuseTickPlantsStep(const PlantShape& s, int substeps) {
  int nrec = 0;
  Refusal r = RefusePlantStep(s, "mpc_batch_tick_plants", substeps, nullptr, 0, false, &nrec);
  if (r.rc && s.plants_begun && s.plant_mode != IDTO_PLANT_PD_PLUS)
    r.msg = "mpc_batch_tick_plants: the plants track the stored plans: idto_hip_plant_begin with IDTO_PLANT_PD_PLUS";
  return r;
}

Refusal RefuseForwardDynamics(const PlantShape& s, const double* x, const double* tau_applied, const double* a_out) {
  const char* who = "forward_dynamics";
  REFUSE_IF(!x || !tau_applied || !a_out, "x[batch][nq + nv], tau_applied[batch][nv] and a_out[batch][nv] are required");
  return Serves(s, who);
}

Refusal RefuseSceneReport(const PlantShape& s, int nstates, const double* x, int models, unsigned mask) {
  const char* who = "scene_report";
  REFUSE_IF(!x, "x[batch][nstates][nq + nv] is required");
  REFUSE_IF(nstates < 1, "nstates must be >= 1");
  REFUSE_IF(!mask, "every output is NULL: nothing to report");
  PASS(Models(s, who, models));
  REFUSE_IF(nstates > (1 << 20), "more than 1048576 states in one call");
  const size_t B = (size_t)s.batch, S = (size_t)nstates, w = (size_t)(s.nq + s.nv);
  for (size_t b = 0; b < B; ++b)
    for (size_t t = 0; t < S; ++t)
      for (size_t i = 0; i < w; ++i)
        REFUSE_IF(!std::isfinite(x[(b * S + t) * w + i]),
                  "x is not finite at problem " + std::to_string(b) + ", state " + std::to_string(t) + ", index " + std::to_string(i));
  REFUSE_IF(idto_dev::scene_lds_doubles(s.nb, s.nq, s.nv, s.npairs, s.blob_n) * sizeof(double) > (size_t)kPlantMaxLds,
            "the model, its bodies' records and its pairs' rows do not fit the 160 KiB of LDS");
  return {};
}

Refusal RefuseLin(const PlantShape& s, const char* who, int nstates, const double* x, const double* tau, double h, int substeps, double eps,
                  int models, const LinTv* tv) {
  REFUSE_IF(!x || !tau, "x[batch][nstates][nq + nv] and tau[batch][nstates][nv] are required");
  REFUSE_IF(nstates < 1, "nstates must be >= 1");
  PASS(Substeps(who, substeps));
  PASS(StepH(who, h));
  REFUSE_IF(!(eps > 0.0) || !std::isfinite(eps), "eps must be > 0 and finite");
  PASS(Models(s, who, models));
  PASS(NoChildren(s, who));
  PASS(Serves(s, who));
  const long long columns = (long long)nstates * lin_columns(s.nv);
  REFUSE_IF(columns > IDTO_LIN_MAX_COLUMNS,
            "nstates * (1 + 6 nv) = " + std::to_string(columns) + " columns, more than " + std::to_string(IDTO_LIN_MAX_COLUMNS) + " in one call");
  const size_t B = (size_t)s.batch, S = (size_t)nstates, nv = (size_t)s.nv, w = (size_t)(s.nq + s.nv), n = 2 * nv;
  if (tv) {
    const size_t nu = (size_t)tv->nu;
    PASS(NuRange(s, who, tv->nu));
    REFUSE_IF(!tv->actuated || !tv->Q || !tv->R || !tv->Qf, "actuated[nu], Q[n * n], R[nu * nu] and Qf[n * n] are required");
    PASS(Actuated(s, who, tv->nu, tv->actuated));
    PASS(Finite(who, "Q", tv->Q, n * n));
    PASS(Finite(who, "R", tv->R, nu * nu));
    PASS(Finite(who, "Qf", tv->Qf, n * n));
    REFUSE_IF(idto_dev::tvlqr_lds_doubles((int)n, (int)nu) * sizeof(double) > (size_t)kPlantMaxLds,
              "the Riccati step's matrices (5 n^2 + 4 n nu + 2 nu^2 + nu doubles, n = 2 nv) do not fit the 160 KiB of LDS");
  }
  PASS(Finite(who, "x", x, B * S * w));
  PASS(Finite(who, "tau", tau, B * S * nv));
  REFUSE_IF(PlantLdsBytes(s, PlantBlock(s, 0, 0), 0) > kPlantMaxLds, "the model and a substep's evaluations do not fit the 160 KiB of LDS");
  return {};
}

Refusal RefuseTrack(const PlantShape& s, const char* who, const TrackCall& a, bool own_K, const double* K) {
  REFUSE_IF(a.S < 1, "nsteps must be >= 1");
  REFUSE_IF(a.R < 1, "nrollouts must be >= 1");
  REFUSE_IF(!a.x_nom || !a.tau_nom || !a.x0 || !a.actuated || (own_K && !K),
            std::string("x_nom[batch][nsteps + 1][nq + nv], tau_nom[batch][nsteps][nv], x0[batch][nrollouts][nq + nv], actuated[nu]") +
                (own_K ? " and K[batch][nsteps][nu * n]" : "") + " are required");
  const long long rollouts = (long long)s.batch * a.R;
  REFUSE_IF(rollouts > IDTO_TRACK_MAX_ROLLOUTS,
            "batch * nrollouts = " + std::to_string(rollouts) + " rollouts, more than " + std::to_string(IDTO_TRACK_MAX_ROLLOUTS) + " in one call");
  PASS(Substeps(who, a.substeps));
  REFUSE_IF(a.max_launch_substeps != 0 && (a.max_launch_substeps < a.substeps || a.max_launch_substeps > IDTO_PLANT_MAX_SUBSTEPS),
            "max_launch_substeps is 0 or in [substeps, 4096] (a launch holds whole control steps)");
  PASS(StepH(who, a.h));
  PASS(Models(s, who, a.models));
  PASS(NoChildren(s, who));
  PASS(Serves(s, who));
  PASS(NuRange(s, who, a.nu));
  PASS(Actuated(s, who, a.nu, a.actuated));
  const size_t B = (size_t)s.batch, S = (size_t)a.S, w = (size_t)(s.nq + s.nv), nv = (size_t)s.nv;
  PASS(Finite(who, "x_nom", a.x_nom, B * (S + 1) * w));
  PASS(Finite(who, "tau_nom", a.tau_nom, B * S * nv));
  PASS(Finite(who, "x0", a.x0, B * (size_t)a.R * w));
  const size_t law = idto_dev::plant_law_doubles(s.nq, s.nv, a.nu);
  REFUSE_IF(PlantLdsBytes(s, PlantBlock(s, 0, law), law) > kPlantMaxLds, "the model, a substep's evaluations and the law's K_t do not fit the 160 KiB of LDS");
  return {};
}

}  // namespace idto_host
