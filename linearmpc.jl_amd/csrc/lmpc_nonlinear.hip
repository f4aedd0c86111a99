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
#include "lmpc_uncertain_host.hpp"

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

// the refusals of lmpc_simulate_scenario_nonlinear*: the program, then all that the uncertain loop refuses (with a
// stand-in for the ignored s->plant), then what joins the two
std::string call_problem(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un,
                         const lmpc_plant_program *prog, const double *q, const double *x, const double *xhat, const double *uprev,
                         bool device) {
    std::string msg = program_problem(prog);
    if (!msg.empty()) return msg;
    if (!s) return "s: NULL descriptor";
    static const double ignored_plant = 0.0;
    lmpc_scenario_sim sc = *s;
    if (!sc.plant) sc.plant = &ignored_plant;
    const HandleObserver ob(h);
    msg = uncertain_problem(h->P.nth, h->P.nout, ob.ptr, &sc, un);
    if (!msg.empty()) return msg;
    if (un->n_plants > 0) return "n_plants: a plant table is not available with a plant program (q takes its place)";
    if (prog->nx != s->nx) return "prog.nx: must equal the descriptor's nx = " + std::to_string(s->nx) + ", got " + std::to_string(prog->nx);
    if (prog->nu != s->nu) return "prog.nu: must equal the descriptor's nu = " + std::to_string(s->nu) + ", got " + std::to_string(prog->nu);
    if (prog->nd != s->nd) return "prog.nd: must equal the descriptor's nd = " + std::to_string(s->nd) + ", got " + std::to_string(prog->nd);
    msg = call_size_problem(N, T, x, un);
    if (!msg.empty()) return msg;
    if (N > 0 && prog->nq > 0 && !q) return "q: NULL with nq > 0";
    return call_array_problem(N, s, xhat, uprev, device);
}

const lmpc_uncertainty no_uncertainty{};


// the run itself, on device arrays, once the call has passed its refusals
int run(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un, const lmpc_plant_program *prog,
        const double *q, int q_shared, double *x, double *xhat, double *uprev, double *U_traj, double *X_traj, int32_t *flag_min,
        hipStream_t st) {
    { const int rce = api_ensure_sim(h, N); if (rce != LMPC_OK) return rce; }
    const int nx = s->nx;
    std::vector<double> hostC;
    ScnConst K = pack_constants(hostC, nx, s->nu, s->nd, s->ny, nullptr, s->measurement, s->cost);    // no plant rows: the program steps x
    UncStep U = pack_uncertainty(hostC, un, nx);
    const ProgOffsets po = pack_program(hostC, prog);
    { const int rcu = upload_constants(h, hostC, K, st); if (rcu != LMPC_OK) return rcu; }
    PlantProg P{}; NlPlant Q{};
    device_program(K.c, po, prog, q, q_shared, P, Q);
    ScnPre A; ScnPost B;
    { const int rcb = scn_begin(h, h->scnScr, N, s, x, xhat, uprev, X_traj, flag_min, h->simTheta, h->simU, h->simFlag, st, A, B);
      if (rcb != LMPC_OK) return rcb; }
    const bool gauss = unc_gauss(U), wantCost = scn_want_cost(s);
    const unsigned gridPost = (unsigned)((N + NL_LANES - 1) / NL_LANES);
    const size_t lds = slot_bytes(prog);
    return scn_loop(h, s, N, T, U_traj, X_traj, A, B,
        [&](int k) {
            unc_advance(U, un, N, nx, k);
            launch_uncertain_pre(N, A, K, U, st);
        },
        [&](int k) { return scn_solve(h, s, N, k, st); },
        [&](int) {
            dispatch_nx(nx, [&](auto NX) {
                if (gauss && wantCost) hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, true, true>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
                else if (gauss) hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, false, true>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
                else if (wantCost) hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, true>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
                else hipLaunchKernelGGL((nonlinear_post_kernel<decltype(NX)::value, false>), dim3(gridPost), dim3(NL_LANES), lds, st, B, K, U, P, Q);
            });
        });
}

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
    return run(h, N, T, s, un, prog, q, q_shared, x, xhat, uprev, U_traj, X_traj, flag_min, (hipStream_t)stream);
}

int lmpc_simulate_scenario_nonlinear(lmpc_handle *h, int64_t N, int T, const lmpc_scenario_sim *s, const lmpc_uncertainty *un,
                                     const lmpc_plant_program *prog, const double *q, int q_shared, double *x, double *xhat,
                                     double *uprev, double *U_traj, double *X_traj, int32_t *flag_min) {
    if (!h) return LMPC_ERR_BADARG;
    if (!un) un = &no_uncertainty;
    // the refusals first, on the caller's descriptor: nothing is allocated for a call that cannot run
    const std::string msg = call_problem(h, N, T, s, un, prog, q, x, xhat, uprev, false);
    if (!msg.empty()) return fail(h, LMPC_ERR_BADARG, "lmpc_simulate_scenario_nonlinear: " + msg);
    if (N == 0 || T == 0) return LMPC_OK;
    LMPC_NEED_DEVICE(h);
    LMPC_ENTER_DEVICE(h);
    Staging sg;
    const StagedScenario g = stage_scenario(sg, N, T, s, x, xhat, uprev, U_traj, X_traj, flag_min);
    const lmpc_uncertainty du = stage_uncertainty(sg, un, N, T, s->nx);
    const double *dq = prog->nq > 0 ? static_cast<const double *>(sg.in(q, sizeof(double) * (q_shared ? 1 : (size_t)N) * prog->nq)) : nullptr;
    if (sg.err != hipSuccess) return sg.fail(h);
    const int rc = run(h, N, T, &g.d, &du, prog, dq, q_shared, g.x, g.xhat, g.uprev, g.U, g.X, g.flag_min, nullptr);
    if (rc == LMPC_OK && (!sg.ok(hipDeviceSynchronize(), "hipDeviceSynchronize") || !sg.download_all())) return sg.fail(h);
    return rc;
}

}  // extern "C"
