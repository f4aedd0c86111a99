// C ABI of liblmpc_hip.so, the nonlinear true plant: lmpc_plant_program_check, the interpreter on the CPU and on the
// device for one plant step, and lmpc_simulate_scenario_nonlinear* -- lmpc_uncertain.hip's loop with its POST kernel's
// plant row sums replaced by the plant program (lmpc_nonlinear_kernels.hpp).  Per step the uncertain loop's PRE kernel,
// the handle's solve (api_launch), the new POST kernel; nothing but enqueues on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "lmpc_internal.hpp"
#include "lmpc_nonlinear_kernels.hpp"
#include "lmpc_scenario_host.hpp"

using namespace lmpc;

namespace {

// how many slot operands an operation reads; -1: unknown opcode
int slot_operands(int op) {
    switch (op) {
        case LMPC_PLANT_LOADX: case LMPC_PLANT_LOADU: case LMPC_PLANT_LOADD: case LMPC_PLANT_LOADQ: case LMPC_PLANT_CONST: return 0;
        case LMPC_PLANT_NEG: case LMPC_PLANT_ABS: case LMPC_PLANT_SIN: case LMPC_PLANT_COS: return 1;
        case LMPC_PLANT_ADD: case LMPC_PLANT_SUB: case LMPC_PLANT_MUL: case LMPC_PLANT_DIV: case LMPC_PLANT_MIN: case LMPC_PLANT_MAX: return 2;
        case LMPC_PLANT_FMA: return 3;
        default: return -1;
    }
}

// Every index the interpreter will form, checked once on the host; "" = fine, otherwise the text, the field's name first.
// What passes addresses slots 0 .. n_slots - 1, constants 0 .. n_consts - 1 and inputs below the declared widths only,
// and reads no slot that no earlier instruction wrote: the kernels check nothing again.
std::string program_problem(const lmpc_plant_program *p) {
    if (!p) return "prog: NULL program";
    auto bad = [](const std::string &f, const std::string &why) { return f + ": " + why; };
    auto num = [](long long v) { return std::to_string(v); };
    if (p->nx < 1 || p->nx > 32) return bad("nx", "1 <= nx <= 32, got " + num(p->nx));
    if (p->nu < 0 || p->nu > 64) return bad("nu", "0 <= nu <= 64, got " + num(p->nu));
    if (p->nd < 0 || p->nd > 32) return bad("nd", "0 <= nd <= 32, got " + num(p->nd));
    if (p->nq < 0 || p->nq > 32) return bad("nq", "0 <= nq <= 32, got " + num(p->nq));
    if (p->n_slots < 1 || p->n_slots > LMPC_PLANT_MAX_SLOTS)
        return bad("n_slots", "1 <= n_slots <= " + num(LMPC_PLANT_MAX_SLOTS) + ", got " + num(p->n_slots));
    if (p->n_consts < 0 || p->n_consts > LMPC_PLANT_MAX_CONSTS)
        return bad("n_consts", "0 <= n_consts <= " + num(LMPC_PLANT_MAX_CONSTS) + ", got " + num(p->n_consts));
    if (p->n_ins < 0 || p->n_ins > LMPC_PLANT_MAX_INS)
        return bad("n_ins", "0 <= n_ins <= " + num(LMPC_PLANT_MAX_INS) + ", got " + num(p->n_ins));
    if (p->n_consts > 0 && !p->consts) return bad("consts", "NULL with n_consts > 0");
    if (p->n_ins > 0 && !p->ins) return bad("ins", "NULL with n_ins > 0");
    if (!p->out_slot) return bad("out_slot", "NULL");
    bool written[LMPC_PLANT_MAX_SLOTS] = {};
    for (int pc = 0; pc < p->n_ins; pc++) {
        const int32_t *I = p->ins + 5 * (size_t)pc;
        const std::string at = "ins[" + num(pc) + "]";
        const int ns = slot_operands(I[0]);
        if (ns < 0) return bad(at + ".op", "unknown opcode " + num(I[0]));
        if (I[1] < 0 || I[1] >= p->n_slots) return bad(at + ".dst", "slot " + num(I[1]) + " outside 0 .. n_slots - 1 = " + num(p->n_slots - 1));
        const char *names[3] = {".a", ".b", ".c"};
        if (ns == 0) {
            const int lim = I[0] == LMPC_PLANT_LOADX ? p->nx : I[0] == LMPC_PLANT_LOADU ? p->nu : I[0] == LMPC_PLANT_LOADD ? p->nd
                          : I[0] == LMPC_PLANT_LOADQ ? p->nq : p->n_consts;
            const char *what = I[0] == LMPC_PLANT_LOADX ? "nx" : I[0] == LMPC_PLANT_LOADU ? "nu" : I[0] == LMPC_PLANT_LOADD ? "nd"
                             : I[0] == LMPC_PLANT_LOADQ ? "nq" : "n_consts";
            if (I[2] < 0 || I[2] >= lim) return bad(at + ".a", "index " + num(I[2]) + " outside 0 .. " + what + " - 1 = " + num(lim - 1));
        }
        for (int o = 0; o < ns; o++) {
            const int sl = I[2 + o];
            if (sl < 0 || sl >= p->n_slots) return bad(at + names[o], "slot " + num(sl) + " outside 0 .. n_slots - 1 = " + num(p->n_slots - 1));
            if (!written[sl]) return bad(at + names[o], "slot " + num(sl) + " is read before any instruction wrote it");
        }
        for (int o = ns == 0 ? 1 : ns; o < 3; o++)
            if (I[2 + o] != 0) return bad(at + names[o], "unused operand field must be 0, got " + num(I[2 + o]));
        written[I[1]] = true;
    }
    for (int a = 0; a < p->nx; a++) {
        const int sl = p->out_slot[a];
        const std::string at = "out_slot[" + num(a) + "]";
        if (sl < 0 || sl >= p->n_slots) return bad(at, "slot " + num(sl) + " outside 0 .. n_slots - 1 = " + num(p->n_slots - 1));
        if (!written[sl]) return bad(at, "slot " + num(sl) + " is never written");
    }
    return "";
}

std::string eval_problem(const lmpc_plant_program *p, int64_t N, const double *x, const double *u, const double *d, const double *q,
                         const double *xnext) {
    std::string msg = program_problem(p);
    if (!msg.empty()) return msg;
    if (N < 0) return "N: negative";
    if (N == 0) return "";
    if (!x) return "x: NULL";
    if (p->nu > 0 && !u) return "u: NULL with nu > 0";
    if (p->nd > 0 && !d) return "d: NULL with nd > 0";
    if (p->nq > 0 && !q) return "q: NULL with nq > 0";
    if (!xnext) return "xnext: NULL";
    return "";
}

// The program behind the run's constants: [consts | ins | out_slot], the int32 arrays copied bit for bit into the
// doubles that carry them.  Returns the offsets (in doubles) of the three parts.
struct ProgOffsets { int consts, ins, out; };
ProgOffsets pack_program(std::vector<double> &v, const lmpc_plant_program *p) {
    auto put_i32 = [&](const int32_t *src, size_t cnt) {
        const int off = (int)v.size();
        v.resize(v.size() + (cnt + 1) / 2 + 1, 0.0);
        if (cnt) std::memcpy(v.data() + off, src, sizeof(int32_t) * cnt);
        return off;
    };
    ProgOffsets o{};
    o.consts = (int)v.size();
    if (p->n_consts > 0) v.insert(v.end(), p->consts, p->consts + p->n_consts);
    else v.push_back(0.0);
    o.ins = put_i32(p->ins, (size_t)p->n_ins * 5);
    o.out = put_i32(p->out_slot, (size_t)p->nx);
    return o;
}

void device_program(const double *base, const ProgOffsets &o, const lmpc_plant_program *p, const double *q, int q_shared,
                    PlantProg &P, NlPlant &Q) {
    P.ins = reinterpret_cast<const int32_t *>(base + o.ins);
    P.consts = base + o.consts;
    P.n_ins = p->n_ins; P.n_slots = p->n_slots; P.nx = p->nx; P.nu = p->nu; P.nd = p->nd; P.nq = p->nq;
    Q.out_slot = reinterpret_cast<const int32_t *>(base + o.out);
    Q.q = q;
    Q.qstride = q_shared ? 0 : p->nq;
}

size_t slot_bytes(const lmpc_plant_program *p) { return sizeof(double) * NL_LANES * (size_t)p->n_slots; }

// the refusals of lmpc_simulate_scenario_nonlinear*: the program, then all that the uncertain loop refuses (its own
// check, asked with a stand-in for the ignored s->plant), then what joins the two
std::string call_problem(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un,
                         const lmpc_plant_program *prog, const double *q, const double *x, const double *xhat, const double *uprev,
                         bool device) {
    std::string msg = program_problem(prog);
    if (!msg.empty()) return msg;
    if (!s) return "s: NULL descriptor";
    static const double ignored_plant = 0.0;
    lmpc_scenario_sim sc = *s;
    if (!sc.plant) sc.plant = &ignored_plant;
    lmpc_observer od{h->obsNx, h->obsNu, h->obsNd, h->obsNy, nullptr, nullptr, nullptr};
    if (lmpc_scenario_uncertain_check(h->P.nth, h->P.nout, h->obsC ? &od : nullptr, &sc, un) != LMPC_OK) {
        const std::string text = g_setup_err, prefix = "lmpc_scenario_uncertain_check: ";
        return text.compare(0, prefix.size(), prefix) == 0 ? text.substr(prefix.size()) : text;
    }
    if (un->n_plants > 0) return "n_plants: a plant table is not available with a plant program (q takes its place)";
    if (prog->nx != s->nx) return "prog.nx: must equal the descriptor's nx = " + std::to_string(s->nx) + ", got " + std::to_string(prog->nx);
    if (prog->nu != s->nu) return "prog.nu: must equal the descriptor's nu = " + std::to_string(s->nu) + ", got " + std::to_string(prog->nu);
    if (prog->nd != s->nd) return "prog.nd: must equal the descriptor's nd = " + std::to_string(s->nd) + ", got " + std::to_string(prog->nd);
    if (N < 0) return "N: negative";
    if (T < 0) return "T: negative";
    if ((int64_t)un->step_offset + T > 2147483647LL) return "step_offset: step_offset + T exceeds 2^31 - 1";
    if (N > 0 && !x) return "x: NULL";
    if (N > 0 && prog->nq > 0 && !q) return "q: NULL with nq > 0";
    if (device && N > 0 && s->nuprev > 0 && !uprev) return "uprev: NULL with nuprev > 0";
    if (xhat && !s->use_observer) return "xhat: given without use_observer";
    return "";
}

// a source as the kernels take it (lmpc_uncertain.hip's packing; the box goes behind the run's constants)
UncSource pack_source(std::vector<double> &v, const lmpc_noise &n) {
    UncSource S{};
    S.src = to_block(nullptr);
    S.w = n.w; S.drawn = n.lo != nullptr && n.w > 0;
    S.lo = S.span = S.hi = -1;
    if (S.drawn && n.dist == LMPC_NOISE_GAUSSIAN) {        // the means, then the standard deviations
        S.drawn = UNC_GAUSSIAN;
        S.lo = (int)v.size(); v.insert(v.end(), n.lo, n.lo + n.w);
        S.span = S.hi = (int)v.size(); v.insert(v.end(), n.hi, n.hi + n.w);
    } else if (S.drawn) {
        S.lo = (int)v.size(); v.insert(v.end(), n.lo, n.lo + n.w);
        S.span = (int)v.size();
        for (int q = 0; q < n.w; q++) v.push_back(n.hi[q] - n.lo[q]);
        S.hi = (int)v.size(); v.insert(v.end(), n.hi, n.hi + n.w);
    } else if (n.w > 0) {
        S.src = to_block(&n.src);
        S.src.w = n.w;
    }
    return S;
}

const lmpc_uncertainty no_uncertainty{};

}  // namespace

extern "C" {

int lmpc_plant_program_check(const lmpc_plant_program *prog) {
    const std::string msg = program_problem(prog);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_plant_program_check: " + msg);
    return LMPC_OK;
}

int lmpc_plant_program_eval_host(const lmpc_plant_program *prog, int64_t N, const double *x, const double *u, const double *d,
                                 const double *q, int q_shared, double *xnext) {
    const std::string msg = eval_problem(prog, N, x, u, d, q, xnext);
    if (!msg.empty()) return fail(nullptr, LMPC_ERR_BADARG, "lmpc_plant_program_eval_host: " + msg);
    const PlantProg P{prog->ins, prog->consts, prog->n_ins, prog->n_slots, prog->nx, prog->nu, prog->nd, prog->nq};
    double slots[LMPC_PLANT_MAX_SLOTS];
    for (int64_t i = 0; i < N; i++) {
        PlantHostEnv E{x + i * prog->nx, u + i * prog->nu, d + i * prog->nd, q + (q_shared ? 0 : i * prog->nq), slots};
        plant_program_run(P, E);
        for (int a = 0; a < prog->nx; a++) xnext[i * prog->nx + a] = slots[prog->out_slot[a]];
    }
    return LMPC_OK;
}

int lmpc_plant_program_eval_device(lmpc_handle *h, const lmpc_plant_program *prog, int64_t N, const double *x, const double *u,
                                   const double *d, const double *q, int q_shared, double *xnext, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    const std::string msg = eval_problem(prog, N, x, u, d, q, xnext);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_plant_program_eval_device: " + msg);
    if (N == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    std::vector<double> hostC;
    const ProgOffsets o = pack_program(hostC, prog);
    ScnConst K{};
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    PlantProg P{}; NlPlant Q{};
    device_program(K.c, o, prog, q, q_shared, P, Q);
    const unsigned grid = (unsigned)((N + NL_LANES - 1) / NL_LANES);
    hipLaunchKernelGGL(plant_program_eval_kernel, dim3(grid), dim3(NL_LANES), slot_bytes(prog), st, P, Q, x, u, d, xnext, (long long)N);
    HIP_TRY(h, hipGetLastError());
    return LMPC_OK;
}

int lmpc_simulate_scenario_nonlinear_device(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s,
                                            const lmpc_uncertainty *un, const lmpc_plant_program *prog, const double *q,
                                            int q_shared, double *x, double *xhat, double *uprev, double *U_traj,
                                            double *X_traj, int32_t *flag_min, void *stream) {
    if (!h) return LMPC_ERR_BADARG;
    if (!un) un = &no_uncertainty;
    const std::string msg = call_problem(h, N, T, s, un, prog, q, x, xhat, uprev, true);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_nonlinear_device: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    const int nx = s->nx, nu = s->nu, nd = s->nd, ny = s->ny, nup = s->nuprev;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, nu, nd, ny, nullptr, s->measurement, s->cost);    // no plant rows: the program steps x
    UncStep U{};
    U.process = pack_source(hostC, un->process);
    U.meas = pack_source(hostC, un->measurement);
    U.gw = -1;
    if (un->Gw && un->process.w > 0) {
        U.gw = (int)hostC.size();
        hostC.insert(hostC.end(), un->Gw, un->Gw + (size_t)nx * un->process.w);
    }
    U.n_plants = 0;
    U.plant_index = nullptr;
    U.key0 = (uint32_t)(un->seed & 0xffffffffu); U.key1 = (uint32_t)(un->seed >> 32);
    U.goff = (unsigned long long)un->scenario_offset;
    const ProgOffsets po = pack_program(hostC, prog);
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    PlantProg P{}; NlPlant Q{};
    device_program(K.c, po, prog, q, q_shared, P, Q);
    // the instantiations that hold the Gaussian sequence serve a run with such a source, and no other
    const bool gauss = U.process.drawn == UNC_GAUSSIAN || U.meas.drawn == UNC_GAUSSIAN;
    const bool obs = s->use_observer != 0;
    const bool wantCost = s->cost && (s->cost_out || s->violation_out);
    const bool needUlast = wantCost && s->cost_out && s->cost->Rr;
    // per-run scratch: the observer state when the caller keeps none, the previous control of the cost's du term
    const size_t needScr = (size_t)N * ((obs && !xhat ? (size_t)nx : 0) + (needUlast ? (size_t)nu : 0));
    if (needScr > h->scnScrCap) {
        hipFree(h->scnScr); h->scnScr = nullptr; h->scnScrCap = 0;
        HIP_TRY(h, hipMalloc(&h->scnScr, sizeof(double) * needScr));
        h->scnScrCap = needScr;
    }
    double *scr = h->scnScr;
    if (obs && !xhat) {                                // set_state!(mpc, x0), simulation.jl:92
        xhat = scr; scr += (size_t)N * nx;
        HIP_TRY(h, hipMemcpyAsync(xhat, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    }
    double *ulast = needUlast ? scr : nullptr;
    if (X_traj) HIP_TRY(h, hipMemcpyAsync(X_traj, x, sizeof(double) * (size_t)N * nx, hipMemcpyDeviceToDevice, st));
    const size_t obs_nd = (size_t)h->obsNx * (1 + h->obsNx + h->obsNu + h->obsNd);
    const size_t obs_nm = (size_t)h->obsNy * (1 + h->obsNx + h->obsNd);
    ScnPre A{};
    A.x = x; A.xhat = obs ? xhat : nullptr; A.uprev = uprev; A.theta = h->simTheta;
    A.obs_meas = obs ? h->obsC + obs_nd : nullptr; A.obs_kt = obs ? h->obsC + obs_nd + obs_nm : nullptr;
    A.r = to_block(&s->r); A.d = to_block(&s->d); A.p = to_block(&s->p); A.noise = to_block(&s->noise);
    A.nx = nx; A.ny = ny; A.nd = nd; A.nup = nup; A.n = (long long)N;
    ScnPost B{};
    B.x = x; B.xhat = obs ? xhat : nullptr; B.uprev = uprev; B.u = h->simU; B.flag = h->simFlag;
    B.obs_dyn = obs ? h->obsC : nullptr; B.d = A.d; B.r = A.r;
    B.flag_min = flag_min; B.cost = wantCost ? s->cost_out : nullptr; B.viol = wantCost ? s->violation_out : nullptr;
    B.ulast = ulast; B.nx = nx; B.nu = nu; B.nd = nd; B.nup = nup; B.n = (long long)N;
    const unsigned grid = (unsigned)((N + 255) / 256);
    const unsigned gridPost = (unsigned)((N + NL_LANES - 1) / NL_LANES);
    const size_t lds = slot_bytes(prog);
    for (int k = 0; k < T; k++) {
        A.k = k;
        A.r.k0 = A.r.H > 0 ? k + 1 : k;
        A.d.k0 = k; A.p.k0 = k;
        A.ym_out = s->Ym_traj ? s->Ym_traj + (size_t)k * N * ny : nullptr;
        A.y_out = s->Y_traj ? s->Y_traj + (size_t)k * N * ny : nullptr;
        A.xhat_out = s->Xhat_traj ? s->Xhat_traj + (size_t)k * N * nx : nullptr;
        A.d_out = s->D_traj ? s->D_traj + (size_t)k * N * nd : nullptr;
        U.step = (uint32_t)(un->step_offset + k);
        U.w_out = un->W_traj ? un->W_traj + (size_t)k * N * nx : nullptr;
        dispatch_nx(nx, [&](auto NX) {
            if (gauss) hipLaunchKernelGGL((uncertain_pre_kernel<decltype(NX)::value, true>), dim3(grid), dim3(256), sizeof(double) * 256 * (size_t)nx, st, A, K, U);
            else hipLaunchKernelGGL(uncertain_pre_kernel<decltype(NX)::value>, dim3(grid), dim3(256), sizeof(double) * 256 * (size_t)nx, st, A, K, U);
        });
        HIP_TRY(h, hipGetLastError());
        const uint64_t *wm = (s->warm && k > 0) ? h->simAct : nullptr;
        const int rc = api_launch(h, N, h->simTheta, h->simU, h->simFlag, nullptr, s->warm ? h->simAct : nullptr, wm, st);
        if (rc != LMPC_OK) return rc;
        B.k = k; B.first = k == 0; B.last = k == T - 1;
        B.xtraj_next = X_traj ? X_traj + (size_t)(k + 1) * N * nx : nullptr;
        B.utraj = U_traj ? U_traj + (size_t)k * N * nu : nullptr;
        dispatch_nx(nx, [&](auto NX) {
            if (gauss && wantCost) hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, true, true>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
            else if (gauss) hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, false, true>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
            else if (wantCost) hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, true>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
            else hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, false>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
        });
        HIP_TRY(h, hipGetLastError());
    }
    return LMPC_OK;
}

int lmpc_simulate_scenario_nonlinear(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un,
                                     const lmpc_plant_program *prog, const double *q, int q_shared, double *x, double *xhat,
                                     double *uprev, double *U_traj, double *X_traj, int32_t *flag_min) {
    if (!h) return LMPC_ERR_BADARG;
    if (!un) un = &no_uncertainty;
    {   // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
        const std::string msg = call_problem(h, N, T, s, un, prog, q, x, xhat, uprev, false);
        if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_nonlinear: " + msg);
    }
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    lmpc_uncertainty du = *un;
    const size_t n = (size_t)N;
    for (lmpc_noise *b : {&du.process, &du.measurement}) {
        const bool read = !b->lo && b->src.src && b->w > 0;
        const size_t cnt = read ? (b->src.stride > 0 ? (n - 1) * (size_t)b->src.stride : 0) + (size_t)b->w * b->src.T : 0;
        b->src.src = read ? static_cast<const double *>(sg.in(b->src.src, sizeof(double) * cnt)) : nullptr;
    }
    du.W_traj = (double *)sg.out(un->W_traj, sizeof(double) * T * n * (size_t)s->nx);
    const double *dq = prog->nq > 0 ? static_cast<const double *>(sg.in(q, sizeof(double) * (q_shared ? 1 : n) * prog->nq)) : nullptr;
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = lmpc_simulate_scenario_nonlinear_device(h, N, T, &g.d, &du, prog, dq, q_shared, g.x, g.xhat, g.uprev, g.U, g.X,
                                                           g.flag_min, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

}  // extern "C"
