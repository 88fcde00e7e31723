// bindings/hsad_host.h -- the host classes behind the COMPILED `rela` / `hanalearn` modules (bindings/rela_module.cc,
// bindings/hanalearn_module.cc): what a maintainer of the reference puts in place of cpp/pybind.cc:14-56 and rela/pybind.cc:16-93 to run
// pyhanabi/create.py / selfplay.py / eval.py on libhsad.so.  Only the C ABI of include/hsad.h is used (plus the HIP runtime for the
// buffers this host owns and a rollout stream); tensors cross the boundary as torch objects created through the interpreter -- no torch
// headers, no ATen ABI.  Same class names and constructor signatures as the reference's bindings:
//
//   hanalearn.HanabiEnv(params, eps, max_len, sad, shuffle_obs, shuffle_color, verbose)      cpp/pybind.cc:15-38
//   hanalearn.HanabiVecEnv().append(env)                                                       cpp/pybind.cc:40-43
//   hanalearn.HanabiThreadLoop(actor | [actors], vec_env, eval)                                cpp/pybind.cc:45-55
//   rela.RNNPrioritizedReplay(capacity, seed, alpha, beta, prefetch) .size .num_add .sample .update_priority   rela/pybind.cc:46-58
//   rela.Context() .push_env_thread .start .pause .resume .terminate .terminated               rela/pybind.cc:62-70
//   rela.R2D2Actor(runner, multi_step, batchsize, gamma, eta, seq_len, num_player, replay) | (runner, num_player)   rela/pybind.cc:72-84
//   rela.BatchRunner(agent, device, max_batch, methods) .start .stop .update_model             rela/pybind.cc:86-90
//   rela.aggregate_priority                                                                    rela/pybind.cc:92
//
// What differs underneath is what differs in the Python mirror (hanabi_sad_amd/rela.py, hanalearn.py): the games of the vector envs a
// Context is given live in ONE batched device env per group of loops that continue each other's seed range and share runner and replay;
// a training loop is hsad_actor_step (cpp/thread_loop.h:42-88 for all games in one call), driven by ONE C++ thread per Context that
// FREE-RUNS like the reference's (rela/context.h:43-50: no pacing in this face), its host at most three steps ahead of the device.
#pragma once
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "hsad.h"

namespace hsadpy {
namespace py = pybind11;

inline void ck(int rc) {
  if (rc) throw std::runtime_error(std::string("libhsad: ") + hsad_last_error());
}
inline void hipck(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
inline int device_index(const std::string& dev) {      // "cuda:1" -> 1, "cuda" -> the current device
  const auto p = dev.find(':');
  if (dev.compare(0, 4, "cuda") != 0) throw std::runtime_error("the device pipeline needs a ROCm device (\"cuda:N\"), not \"" + dev + "\"");
  if (p == std::string::npos) {
    int d = 0;
    hipck(hipGetDevice(&d), "hipGetDevice");
    return d;
  }
  return std::stoi(dev.substr(p + 1));
}
// the stream torch's caller is on (kernels of calls made from Python order with the surrounding PyTorch work)
inline void* torch_stream(int device) {
  py::object s = py::module_::import("torch").attr("cuda").attr("current_stream")(device);
  return reinterpret_cast<void*>(s.attr("cuda_stream").cast<uintptr_t>());
}
struct DevBuf {      // device memory this host owns (zero-filled)
  void* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void alloc(size_t bytes) {
    release();
    n = bytes ? bytes : 16;
    hipck(hipMalloc(&p, n), "hipMalloc");
    hipck(hipMemset(p, 0, n), "hipMemset");
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
  }
  ~DevBuf() { release(); }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

struct EnvCfg {
  int players = 2, hand = 5, seed = 1, bomb = 0, max_len = 80;
  bool sad = false, shuffle_obs = false, shuffle_color = false;
  hsad_env_rules rules{5, 5, 8, 3};   // HLE colors / ranks / max_information_tokens / max_life_tokens
  std::vector<float> eps;
  bool same_but_seed(const EnvCfg& o) const {
    return players == o.players && hand == o.hand && bomb == o.bomb && max_len == o.max_len && sad == o.sad && shuffle_obs == o.shuffle_obs &&
           shuffle_color == o.shuffle_color && eps == o.eps && rules.colors == o.rules.colors && rules.ranks == o.rules.ranks &&
           rules.max_information_tokens == o.rules.max_information_tokens && rules.max_life_tokens == o.rules.max_life_tokens;
  }
};

// ---- one batched device env: hsad_env + the buffers bound to it ----
struct BatchedEnv {
  hsad_env* h = nullptr;
  int G = 0, P = 0, F = 0, A = 0, H = 0, device = 0, Fp = 0;
  DevBuf priv_s, legal, own, eps, reward, terminal, priv_bits, legal_bits, own_bits, priv_bf16, query;
  std::vector<int32_t> q_host;
  std::mutex q_mu;
  BatchedEnv(int games, const EnvCfg& c, int dev, bool deck_history) : G(games), device(dev) {
    hipck(hipSetDevice(dev), "hipSetDevice");
    hsad_env_config k{};
    k.num_games = games;
    k.players = c.players;
    k.hand_size = c.hand;
    k.bomb = c.bomb;
    k.seed0 = c.seed;
    k.max_len = c.max_len;
    k.sad = c.sad;
    k.shuffle_obs = c.shuffle_obs;
    k.shuffle_color = c.shuffle_color;
    k.n_eps = (int)c.eps.size();
    k.eps_list = c.eps.data();
    k.device = dev;
    k.track_deck_history = deck_history;
    ck(hsad_env_create_rules(&k, &c.rules, &h));
    P = hsad_env_num_players(h);
    F = hsad_env_feature_size(h);
    A = hsad_env_num_action(h);
    H = c.hand;
    const size_t N = (size_t)G * P;
    priv_s.alloc(N * F * 4);
    legal.alloc(N * A * 4);
    own.alloc(N * 3 * H * 4);
    eps.alloc(N * 4);
    reward.alloc((size_t)G * 4);
    terminal.alloc(G);
    query.alloc((size_t)G * HSAD_QUERY_WORDS * 4);
    q_host.resize((size_t)G * HSAD_QUERY_WORDS);
    ck(hsad_env_bind_outputs(h, priv_s.as<float>(), legal.as<float>(), own.as<float>(), eps.as<float>(), reward.as<float>(), terminal.as<uint8_t>()));
  }
  // packed outputs for the device actor / the acting net (hsad_env_bind_packed); the float32 observation is then no longer written unless
  // keep_float32 (a contract model of an evaluation loop reads it)
  void enable_packed(int row_len, bool keep_float32 = false) {
    const size_t N = (size_t)G * P;
    Fp = row_len;
    priv_bits.alloc(N * ((F + 63) / 64) * 8);
    legal_bits.alloc(N * 8);
    own_bits.alloc(N * 8);
    priv_bf16.alloc(N * (size_t)row_len * 2);
    ck(hsad_env_bind_packed(h, priv_bits.as<uint64_t>(), legal_bits.as<uint64_t>(), own_bits.as<uint64_t>(), priv_bf16.p, row_len, keep_float32 ? 1 : 0));
  }
  std::vector<int32_t> read_query(void* stream) {      // per-game scalars on the host (synchronises the stream)
    std::lock_guard<std::mutex> g(q_mu);
    ck(hsad_env_query(h, query.as<int32_t>(), stream));
    hipck(hipMemcpyAsync(q_host.data(), query.p, q_host.size() * 4, hipMemcpyDeviceToHost, (hipStream_t)stream), "hipMemcpyAsync");
    hipck(hipStreamSynchronize((hipStream_t)stream), "hipStreamSynchronize");
    return q_host;
  }
  ~BatchedEnv() {
    if (h) hsad_env_destroy(h);
  }
};

class HanabiVecEnv;

// hanalearn.HanabiEnv: one game.  Standalone it is a 1-game device env; appended to a vector env it is a row of that env's batch.
class HanabiEnv {
 public:
  EnvCfg cfg;
  std::shared_ptr<BatchedEnv> own;           // standalone 1-game env (created on first use)
  std::shared_ptr<BatchedEnv> batch;         // the batch this game lives in once a Context has built it
  int row = 0;
  HanabiEnv(const std::unordered_map<std::string, std::string>& params, const std::vector<float>& eps, int max_len, bool sad, bool shuffle_obs,
            bool shuffle_color, bool verbose) {
    auto get = [&](const char* k, int dflt) {
      auto it = params.find(k);
      return it == params.end() ? dflt : std::stoi(it->second);
    };
    cfg.players = get("players", 2);
    cfg.hand = get("hand_size", 5);
    cfg.seed = get("seed", 1);
    cfg.bomb = get("bomb", 0);
    // HLE's game keys: the rules are honoured within their bounds, the rest refused unless at HLE's default (hanalearn.game_rules)
    auto rule = [&](const char* k, int dflt, int lo, int hi) {
      const int v = get(k, dflt);
      if (v < lo || v > hi)
        throw std::invalid_argument(std::string("HanabiEnv: ") + k + " must be " + std::to_string(lo) + ".." + std::to_string(hi) +
                                    " (got " + std::to_string(v) + ")");
      return v;
    };
    cfg.rules.colors = rule("colors", 5, 1, 5);
    cfg.rules.ranks = rule("ranks", 5, 1, 5);
    cfg.rules.max_information_tokens = rule("max_information_tokens", 8, 1, 8);
    cfg.rules.max_life_tokens = rule("max_life_tokens", 3, 1, 3);
    if (get("observation_type", 1) != 1)
      throw std::invalid_argument("HanabiEnv: observation_type " + params.at("observation_type") + " is not supported (only 1, card knowledge)");
    {
      auto it = params.find("random_start_player");
      // the values accepted as "off", exactly: the same as hanalearn.RANDOM_START_OFF of the Python face
      if (it != params.end() && it->second != "0" && it->second != "false" && it->second != "False")
        throw std::invalid_argument("HanabiEnv: random_start_player is not supported (got " + it->second + ")");
    }
    cfg.max_len = max_len;
    cfg.sad = sad;
    cfg.shuffle_obs = shuffle_obs;
    cfg.shuffle_color = shuffle_color;
    cfg.eps = eps;
    if (verbose) py::print("Hanabi game created, players", cfg.players, "hand_size", cfg.hand, "seed", cfg.seed, "bomb", cfg.bomb);
  }
  BatchedEnv& single() {
    if (!own) {
      int d = 0;
      hipck(hipGetDevice(&d), "hipGetDevice");
      own = std::make_shared<BatchedEnv>(1, cfg, d, true);
    }
    return *own;
  }
  int feature_size() { return batch ? batch->F : single().F; }
  int num_action() { return batch ? batch->A : single().A; }
  int hand_feature_size() { return hsad_env_hand_feature_size(batch ? batch->h : single().h); }
  int q(int word) {
    BatchedEnv& e = batch ? *batch : single();
    const int r = batch ? row : 0;
    return e.read_query(torch_stream(e.device))[(size_t)r * HSAD_QUERY_WORDS + word];
  }
  bool terminated() { return q(HSAD_Q_TERMINATED) != 0; }
  int get_current_player() { return q(HSAD_Q_CUR_PLAYER); }
  int get_score() { return q(HSAD_Q_SCORE); }
  int get_life() { return q(HSAD_Q_LIFE); }
  int get_info() { return q(HSAD_Q_INFO); }
  int last_score() { return q(HSAD_Q_LAST_SCORE); }
  std::vector<int> get_fireworks() {
    BatchedEnv& e = batch ? *batch : single();
    const auto v = e.read_query(torch_stream(e.device));
    const size_t o = (size_t)(batch ? row : 0) * HSAD_QUERY_WORDS + HSAD_Q_FIREWORKS;
    return {v[o], v[o + 1], v[o + 2], v[o + 3], v[o + 4]};
  }
  // ---- single-game driving (cpp/hanabi_env.cc:9-113), on the game's own 1-game env like the Python face's (hanalearn.py:65-122) ----
  // {priv_s [P, F], legal_move [P, A], eps [P], own_hand [P, 3 * hand]}: float32 copies of the env's outputs on the game's device
  py::dict obs_copy(BatchedEnv& e, void* stream) {
    py::object torch = py::module_::import("torch");
    py::object dev = torch.attr("device")("cuda", e.device);
    py::dict d;
    auto copy = [&](const char* name, const DevBuf& src, std::vector<int64_t> shape) {
      size_t n = 1;
      for (auto s : shape) n *= (size_t)s;
      py::object t = torch.attr("empty")(py::cast(shape), py::arg("dtype") = torch.attr("float32"), py::arg("device") = dev);
      hipck(hipMemcpyAsync(reinterpret_cast<void*>(t.attr("data_ptr")().cast<uintptr_t>()), src.p, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream),
            "hipMemcpyAsync");
      d[py::str(name)] = t;
    };
    copy("priv_s", e.priv_s, {e.P, e.F});
    copy("legal_move", e.legal, {e.P, e.A});
    copy("eps", e.eps, {e.P});
    copy("own_hand", e.own, {e.P, 3 * e.H});
    return d;
  }
  py::dict reset() {
    BatchedEnv& e = single();
    hipck(hipSetDevice(e.device), "hipSetDevice");
    void* s = torch_stream(e.device);
    ck(hsad_env_reset(e.h, s));
    return obs_copy(e, s);
  }
  // action: {"a": int64 [P], "greedy_a": int64 [P] (optional)} -> (obs, reward, terminal).  An illegal move or a step on a finished game
  // raises (the reference asserts, hanabi_env.cc:63-80); the library has left the game untouched.
  py::tuple step(const py::dict& action) {
    BatchedEnv& e = single();
    hipck(hipSetDevice(e.device), "hipSetDevice");
    py::object torch = py::module_::import("torch");
    py::object dev = torch.attr("device")("cuda", e.device);
    auto column = [&](const char* key) {
      py::object t = action[py::str(key)].attr("to")(dev, torch.attr("int64")).attr("reshape")(-1).attr("contiguous")();
      if (t.attr("numel")().cast<int64_t>() != e.P)
        throw std::invalid_argument(std::string("HanabiEnv.step: action[\"") + key + "\"] must hold one move per player (" + std::to_string(e.P) + ")");
      return t;
    };
    py::object a = column("a");
    py::object g = action.contains(py::str("greedy_a")) ? column("greedy_a") : (cfg.sad ? a : py::object(py::none()));
    auto ptr = [](const py::object& t) { return reinterpret_cast<const int64_t*>(t.attr("data_ptr")().cast<uintptr_t>()); };
    void* s = torch_stream(e.device);
    ck(hsad_env_step(e.h, ptr(a), g.is_none() ? nullptr : ptr(g), s));
    int32_t n = 0, first = 0, code = 0;
    {
      py::gil_scoped_release nogil;
      ck(hsad_env_error_count(e.h, &n, &first, &code));      // (synchronises the device)
    }
    if (n) {
      const char* what = code == 1 ? "illegal move" : code == 2 ? "illegal greedy move" : code == 3 ? "step on a finished game" : "?";
      throw std::runtime_error(std::to_string(n) + " game(s) violated the env contract; first: game " + std::to_string(first) + ", " + what);
    }
    py::dict obs = obs_copy(e, s);
    float reward = 0.f;
    uint8_t terminal = 0;
    hipck(hipMemcpyAsync(&reward, e.reward.p, 4, hipMemcpyDeviceToHost, (hipStream_t)s), "hipMemcpyAsync");
    hipck(hipMemcpyAsync(&terminal, e.terminal.p, 1, hipMemcpyDeviceToHost, (hipStream_t)s), "hipMemcpyAsync");
    hipck(hipStreamSynchronize((hipStream_t)s), "hipStreamSynchronize");
    return py::make_tuple(obs, reward, terminal != 0);
  }
  // HanabiEnv::moveIsLegal: the game where the queries read it (its vector env's batch once built, else the 1-game env)
  bool move_is_legal(int uid) {
    BatchedEnv& e = batch ? *batch : single();
    const int r = batch ? row : 0;
    hipck(hipSetDevice(e.device), "hipSetDevice");
    py::object torch = py::module_::import("torch");
    py::object dev = torch.attr("device")("cuda", e.device);
    py::object u = torch.attr("full")(py::make_tuple(e.G), uid, py::arg("dtype") = torch.attr("int32"), py::arg("device") = dev);
    std::vector<uint8_t> out((size_t)e.G);
    DevBuf d;
    d.alloc((size_t)e.G);
    void* s = torch_stream(e.device);
    ck(hsad_env_move_is_legal(e.h, reinterpret_cast<const int32_t*>(u.attr("data_ptr")().cast<uintptr_t>()), d.as<uint8_t>(), s));
    hipck(hipMemcpyAsync(out.data(), d.p, out.size(), hipMemcpyDeviceToHost, (hipStream_t)s), "hipMemcpyAsync");
    hipck(hipStreamSynchronize((hipStream_t)s), "hipStreamSynchronize");
    return out[(size_t)r] != 0;
  }
  // HanabiEnv::deckHistory (cpp/hanabi_env.h:112-114): the dealt cards of the 1-game env's episode as "R1" (colour letter + rank)
  std::vector<std::string> deck_history() {
    BatchedEnv& e = single();
    hipck(hipSetDevice(e.device), "hipSetDevice");
    DevBuf cards, count;
    cards.alloc(50);
    count.alloc(4);
    void* s = torch_stream(e.device);
    ck(hsad_env_deck_history(e.h, cards.as<uint8_t>(), count.as<int32_t>(), s));
    uint8_t c[50];
    int32_t n = 0;
    hipck(hipMemcpyAsync(c, cards.p, 50, hipMemcpyDeviceToHost, (hipStream_t)s), "hipMemcpyAsync");
    hipck(hipMemcpyAsync(&n, count.p, 4, hipMemcpyDeviceToHost, (hipStream_t)s), "hipMemcpyAsync");
    hipck(hipStreamSynchronize((hipStream_t)s), "hipStreamSynchronize");
    std::vector<std::string> out;
    for (int i = 0; i < n && i < 50; ++i) {
      if (c[i] >= 25) throw std::runtime_error("HanabiEnv.deck_history: card code out of range");
      out.push_back(std::string(1, "RYGWB"[c[i] / 5]) + std::to_string(c[i] % 5 + 1));
    }
    return out;
  }
};

class HanabiVecEnv {
 public:
  std::vector<std::shared_ptr<HanabiEnv>> envs;
  void append(std::shared_ptr<HanabiEnv> e) { envs.push_back(std::move(e)); }
  int size() const { return (int)envs.size(); }
};

// ---- rela.BatchRunner: the model behind the actors = two hsad_r2d2_net (online, target) loaded from agent.state_dict(), or -- for a model
// that is not the R2D2Net shape but implements act / get_h0 (on agent._c for a TorchScript wrapper, rela/batch_runner.h:24,108) -- that
// model itself, called from the loop thread (a contract runner: evaluation loops only; rela.BatchRunner.update_model of the Python face)
//
// Locks: the GIL, then `mu`, never the other way round.  Nobody blocks on `mu` while holding the GIL: the kernel path gathers its tensors
// under the GIL and copies them with the GIL released; the contract path (which needs the GIL for the model) only try-locks `mu` and lets
// the GIL go between attempts (lock_with_gil).
class BatchRunner {
 public:
  py::object agent;
  std::string device_str;
  int device = 0;
  hsad_r2d2_net *online = nullptr, *target = nullptr;
  int in_dim = 0, hid = 0, num_action = 0, hand = 0, nfc = 1, nl = 2;
  bool skip_connect = false;      // R2D2Net.skip_connect (pyhanabi/r2d2.py:74): read off agent.online_net when it is there
  bool contract = false;          // the model is called as it is (act / get_h0), no kernels
  py::object impl;                // contract: getattr(agent, "_c", agent)
  std::mutex mu;      // update_model vs the loop thread's steps (BatchRunner::updateModel takes the model lock, rela/batch_runner.h:74-77)
  BatchRunner(py::object ag, const std::string& dev, int /*max_batch*/, const std::vector<std::string>& /*methods*/)
      : agent(std::move(ag)), device_str(dev), device(device_index(dev)) {
    build();
  }
  ~BatchRunner() {
    if (online) hsad_r2d2_net_destroy(online);
    if (target) hsad_r2d2_net_destroy(target);
  }
  void start() {}
  void stop() {}
  static std::vector<int64_t> shape_of(const py::object& t) { return t.attr("shape").cast<std::vector<int64_t>>(); }
  static bool is_r2d2_shape(const py::dict& sd) {
    const std::string on = "online_net.";
    return sd.contains(py::str(on + "net.0.weight")) && sd.contains(py::str(on + "fc_a.weight")) && sd.contains(py::str(on + "pred.weight"));
  }
  // the GIL is held: take `mu` without ever blocking on it while holding the GIL
  std::unique_lock<std::mutex> lock_with_gil() {
    std::unique_lock<std::mutex> g(mu, std::try_to_lock);
    while (!g.owns_lock()) {
      {
        py::gil_scoped_release nogil;
        std::this_thread::yield();
      }
      g.try_lock();
    }
    return g;
  }
  void build() {
    py::dict sd = py::hasattr(agent, "state_dict") ? py::dict(agent.attr("state_dict")()) : py::dict();
    if (!is_r2d2_shape(sd)) {
      py::object c = py::getattr(agent, "_c", agent);
      if (py::hasattr(c, "act") && py::hasattr(c, "get_h0")) {
        contract = true;
        impl = c;
        return;
      }
      throw std::runtime_error("BatchRunner: agent.state_dict() has no online_net.* of an R2D2Net (net.0 / lstm / fc_v / fc_a / pred), and the "
                               "agent has no act / get_h0 of the model contract");
    }
    const std::string on = "online_net.";
    auto has = [&](const std::string& k) { return sd.contains(py::str(k)); };
    const auto w0 = shape_of(sd[py::str(on + "net.0.weight")]);
    hid = (int)w0[0];
    in_dim = (int)w0[1];
    num_action = (int)shape_of(sd[py::str(on + "fc_a.weight")])[0];
    hand = (int)shape_of(sd[py::str(on + "pred.weight")])[0] / 3;
    nfc = has(on + "net.2.weight") ? 2 : 1;
    nl = 0;
    while (has(on + "lstm.weight_ih_l" + std::to_string(nl))) ++nl;
    if (py::hasattr(agent, "online_net")) skip_connect = py::getattr(agent.attr("online_net"), "skip_connect", py::bool_(false)).cast<bool>();
    hipck(hipSetDevice(device), "hipSetDevice");
    ck(hsad_r2d2_net_create_ex(in_dim, hid, num_action, hand, nfc, nl, skip_connect ? 1 : 0, 0, device, &online));
    ck(hsad_r2d2_net_create_ex(in_dim, hid, num_action, hand, nfc, nl, skip_connect ? 1 : 0, 0, device, &target));
    load(sd);
  }
  struct Staged {      // one parameter tensor, converted under the GIL, copied without it
    py::object t;
    const void* src;
    size_t offset, count;
  };
  std::vector<Staged> stage_net(const py::dict& sd, const std::string& prefix, hsad_r2d2_net* net) {
    py::object f32 = py::module_::import("torch").attr("float32");
    std::vector<Staged> out;
    const int n = hsad_r2d2_net_num_params(net);
    for (int i = 0; i < n; ++i) {
      const std::string key = prefix + hsad_r2d2_net_param_name(net, i);
      if (!sd.contains(py::str(key))) throw std::runtime_error("BatchRunner: state_dict lacks " + key);
      py::object t = sd[py::str(key)].attr("detach")().attr("to")(f32).attr("contiguous")();
      const int64_t want = hsad_r2d2_net_param_size(net, i);
      if (t.attr("numel")().cast<int64_t>() != want) throw std::runtime_error("BatchRunner: " + key + " has the wrong number of elements");
      out.push_back({t, reinterpret_cast<const void*>(t.attr("data_ptr")().cast<uintptr_t>()), (size_t)hsad_r2d2_net_param_offset(net, i), (size_t)want});
    }
    return out;
  }
  static void copy_net(const std::vector<Staged>& st, hsad_r2d2_net* net, void* stream) {
    float* flat = hsad_r2d2_net_params(net);
    // (a synchronous copy: the source may be pageable host memory or a device tensor of any stream)
    for (const auto& s : st) hipck(hipMemcpy(flat + s.offset, s.src, s.count * 4, hipMemcpyDefault), "hipMemcpy(parameters)");
    ck(hsad_r2d2_net_refresh(net, stream));
  }
  void load(const py::dict& sd) {      // (GIL held)
    hipck(hipSetDevice(device), "hipSetDevice");
    py::object torch = py::module_::import("torch");
    torch.attr("cuda").attr("synchronize")(device);
    void* s = torch_stream(device);
    const auto on = stage_net(sd, "online_net.", online);
    const auto tg = stage_net(sd, sd.contains(py::str("target_net.net.0.weight")) ? "target_net." : "online_net.", target);
    py::gil_scoped_release nogil;      // wait for the loop thread's step without the GIL (its contract seats may need it to finish)
    std::lock_guard<std::mutex> g(mu);
    hipck(hipSetDevice(device), "hipSetDevice");
    copy_net(on, online, s);
    copy_net(tg, target, s);
    hipck(hipStreamSynchronize((hipStream_t)s), "hipStreamSynchronize");
  }
  void update_model(py::object ag) {      // BatchRunner::updateModel
    if (!contract) return load(ag.attr("state_dict")());
    if (ag.is(agent)) return;             // the runner calls that very model
    auto g = lock_with_gil();
    agent.attr("load_state_dict")(ag.attr("state_dict")());
  }
};

// rela.RNNTransition: the batch replay.sample returns (fields are torch tensors / dicts of them, rela/pybind.cc:26-33)
struct RNNTransition {
  py::object obs, h0, action, reward, terminal, bootstrap, seq_len;
};

// rela.FFTransition (rela/pybind.cc:17-23, rela/transition.h:16-35): one feed-forward transition batch; nothing in the compiled modules
// produces it (the reference's FFPrioritizedReplay binding is commented out), index / to_dict follow transition.cc and the Python face
struct FFTransition {
  py::object obs, action, reward, terminal, bootstrap, next_obs;
  FFTransition index(int i) const {      // FFTransition::index: element i of every batched field
    auto pick = [i](const py::object& d) {
      py::dict out;
      for (auto kv : d.cast<py::dict>()) out[kv.first] = kv.second.attr("__getitem__")(i);
      return py::object(out);
    };
    return FFTransition{pick(obs), pick(action), reward.attr("__getitem__")(i), terminal.attr("__getitem__")(i), bootstrap.attr("__getitem__")(i),
                        pick(next_obs)};
  }
  py::dict to_dict() const {      // FFTransition::toDict: obs and action keys, `next_`-prefixed next_obs, then the scalars
    py::dict d;
    for (auto kv : obs.cast<py::dict>()) d[kv.first] = kv.second;
    for (auto kv : action.cast<py::dict>()) d[kv.first] = kv.second;
    for (auto kv : next_obs.cast<py::dict>()) d[py::str("next_" + kv.first.cast<std::string>())] = kv.second;
    d["reward"] = reward;
    d["terminal"] = terminal;
    d["bootstrap"] = bootstrap;
    return d;
  }
};

// ---- rela.RNNPrioritizedReplay on hsad_replay (created once the transition layout is known: when its first loop is built) ----
class RNNPrioritizedReplay {
 public:
  int capacity, seed, prefetch;
  float alpha, beta;
  hsad_replay* h = nullptr;
  int device = -1, T = 0;
  struct FieldSpec {
    std::string name;
    int width, dtype, segments;      // dtype: hsad_dtype
  };
  std::vector<FieldSpec> fields;
  RNNPrioritizedReplay(int capacity_, int seed_, float alpha_, float beta_, int prefetch_)
      : capacity(capacity_), seed(seed_), prefetch(prefetch_), alpha(alpha_), beta(beta_) {}
  ~RNNPrioritizedReplay() {
    if (h) hsad_replay_destroy(h);
  }
  // transition layout of a Hanabi actor (hsad_actor_io's comment in include/hsad.h): m = players (VDN) or 1 (IQL)
  void bind_schema(int F, int A, int hand, int m, int seq_len, int dev) {
    std::vector<FieldSpec> f = {{"priv_s", m * F, HSAD_BITS, m},     {"legal_move", m * A, HSAD_BITS, m}, {"eps", m, HSAD_F32, 1},
                                {"own_hand", m * 3 * hand, HSAD_BITS, m}, {"a", m, HSAD_I64, 1},           {"greedy_a", m, HSAD_I64, 1}};
    if (h) {
      bool same = dev == device && seq_len == T && f.size() == fields.size();
      for (size_t i = 0; same && i < f.size(); ++i) same = f[i].width == fields[i].width && f[i].dtype == fields[i].dtype && f[i].segments == fields[i].segments;
      if (!same) throw std::runtime_error("RNNPrioritizedReplay: the loops feeding one replay must share device, sequence length and transition layout");
      return;
    }
    fields = f;
    device = dev;
    T = seq_len;
    std::vector<hsad_field> hf(f.size());
    for (size_t i = 0; i < f.size(); ++i) {
      hf[i].width = f[i].width;
      hf[i].dtype = f[i].dtype == HSAD_BITS ? (HSAD_BITS | (f[i].segments << 8)) : f[i].dtype;
    }
    hipck(hipSetDevice(dev), "hipSetDevice");
    ck(hsad_replay_create(capacity, seed, alpha, beta, prefetch, seq_len, (int)hf.size(), hf.data(), dev, &h));
  }
  std::pair<int, int> counters() {
    if (!h) return {0, 0};
    int32_t size = 0, num_add = 0;
    py::gil_scoped_release nogil;
    ck(hsad_replay_size(h, &size, &num_add));
    return {size, num_add};
  }
  int size() { return counters().first; }
  int num_add() { return counters().second; }
  // PrioritizedReplay::sample -> (RNNTransition of [T, B, ...] tensors on `device`, importance weights [B]); "cpu" = the batch drawn on the
  // replay's device and handed over as CPU tensors (rela/prioritized_replay.h:208,343)
  py::tuple sample(int batch, const std::string& dev) {
    if (!h) throw std::runtime_error("RNNPrioritizedReplay.sample: nothing has been added yet (no loop feeds this replay)");
    const bool to_cpu = dev == "cpu";
    if (!to_cpu && device_index(dev) != device) throw std::runtime_error("RNNPrioritizedReplay.sample: the replay lives on cuda:" + std::to_string(device));
    py::tuple out = sample_device(batch);
    if (!to_cpu) return out;
    auto& b = *out[0].cast<std::shared_ptr<RNNTransition>>();
    auto cpu_dict = [](const py::object& d) {
      py::dict o;
      for (auto kv : d.cast<py::dict>()) o[kv.first] = kv.second.attr("cpu")();
      return py::object(o);
    };
    RNNTransition c{cpu_dict(b.obs), cpu_dict(b.h0), cpu_dict(b.action), b.reward.attr("cpu")(), b.terminal.attr("cpu")(), b.bootstrap.attr("cpu")(),
                    b.seq_len.attr("cpu")()};
    return py::make_tuple(py::cast(std::make_shared<RNNTransition>(std::move(c))), out[1].attr("cpu")());
  }
  // PrioritizedReplay::get (rela/prioritized_replay.h): the idx-th stored sequence counted from the ring head, laid out like the Python
  // face's (hanabi_sad_amd/rela.py RNNPrioritizedReplay.get): obs [T, 1, w], action [T, w], reward / terminal / bootstrap [T], seq_len scalar
  py::object get(int idx) {
    if (!h) throw std::runtime_error("RNNPrioritizedReplay.get: nothing has been added yet (no loop feeds this replay)");
    const int n = size();
    if (idx < 0 || idx >= n)
      throw py::index_error("RNNPrioritizedReplay.get: index " + std::to_string(idx) + " outside the " + std::to_string(n) + " stored sequences");
    hipck(hipSetDevice(device), "hipSetDevice");
    py::object torch = py::module_::import("torch");
    py::object tdev = torch.attr("device")("cuda", device);
    auto empty = [&](std::vector<int64_t> shape, const char* dtype) {
      return torch.attr("empty")(py::cast(shape), py::arg("dtype") = torch.attr(dtype), py::arg("device") = tdev);
    };
    auto ptr = [](const py::object& t) { return reinterpret_cast<void*>(t.attr("data_ptr")().cast<uintptr_t>()); };
    std::vector<py::object> outs;
    std::vector<void*> out_ptrs;
    for (const auto& f : fields) {
      outs.push_back(empty({T, f.width}, f.dtype == HSAD_I64 ? "int64" : "float32"));
      out_ptrs.push_back(ptr(outs.back()));
    }
    py::object reward = empty({T}, "float32"), terminal = empty({T}, "uint8"), bootstrap = empty({T}, "float32"), seq_len = empty({1}, "float32");
    ck(hsad_replay_get(h, idx, out_ptrs.data(), (float*)ptr(reward), (uint8_t*)ptr(terminal), (float*)ptr(bootstrap), (float*)ptr(seq_len),
                       torch_stream(device)));
    py::dict obs, action;
    for (size_t i = 0; i < fields.size(); ++i) {
      const std::string& nm = fields[i].name;
      if (nm == "a" || nm == "greedy_a") action[py::str(nm)] = outs[i];
      else obs[py::str(nm)] = outs[i].attr("unsqueeze")(1);
    }
    RNNTransition b{obs, py::dict(), action, reward, terminal.attr("view")(torch.attr("bool")), bootstrap, seq_len.attr("__getitem__")(0)};
    return py::cast(std::make_shared<RNNTransition>(std::move(b)));
  }
  py::tuple sample_device(int batch) {
    py::object torch = py::module_::import("torch");
    py::object tdev = torch.attr("device")("cuda", device);
    auto empty = [&](std::vector<int64_t> shape, const char* dtype) {
      return torch.attr("empty")(py::cast(shape), py::arg("dtype") = torch.attr(dtype), py::arg("device") = tdev);
    };
    auto ptr = [](const py::object& t) { return reinterpret_cast<void*>(t.attr("data_ptr")().cast<uintptr_t>()); };
    std::vector<py::object> outs;
    std::vector<void*> out_ptrs;
    for (const auto& f : fields) {
      outs.push_back(empty({T, batch, f.width}, f.dtype == HSAD_I64 ? "int64" : "float32"));
      out_ptrs.push_back(ptr(outs.back()));
    }
    py::object reward = empty({T, batch}, "float32"), terminal = empty({T, batch}, "uint8"), bootstrap = empty({T, batch}, "float32");
    py::object seq_len = empty({batch}, "float32"), weight = empty({batch}, "float32");
    ck(hsad_replay_sample(h, batch, out_ptrs.data(), (float*)ptr(reward), (uint8_t*)ptr(terminal), (float*)ptr(bootstrap), (float*)ptr(seq_len),
                          (float*)ptr(weight), torch_stream(device)));
    py::dict obs, action;
    for (size_t i = 0; i < fields.size(); ++i) {
      const std::string& n = fields[i].name;
      if (n == "a" || n == "greedy_a") action[py::str(n)] = outs[i].attr("squeeze")(2);
      else obs[py::str(n)] = n == "eps" ? outs[i].attr("squeeze")(2) : outs[i];
    }
    RNNTransition b{obs, py::dict(), action, reward, terminal.attr("view")(torch.attr("bool")), bootstrap, seq_len};
    return py::make_tuple(py::cast(std::make_shared<RNNTransition>(std::move(b))), weight);
  }
  void update_priority(py::object priority) {
    py::object torch = py::module_::import("torch");
    py::object p = priority.attr("detach")().attr("to")(torch.attr("device")("cuda", device), torch.attr("float32")).attr("contiguous")();
    ck(hsad_replay_update_priority(h, reinterpret_cast<const float*>(p.attr("data_ptr")().cast<uintptr_t>()), (int)p.attr("numel")().cast<int64_t>(),
                                   torch_stream(device)));
  }
};

inline py::object aggregate_priority(py::object priority, py::object seq_len, float eta) {      // rela/r2d2_actor.h:10-21
  py::object torch = py::module_::import("torch");
  const bool on_gpu = priority.attr("is_cuda").cast<bool>();
  int dev = 0;
  if (on_gpu) dev = priority.attr("device").attr("index").cast<int>();
  else hipck(hipGetDevice(&dev), "hipGetDevice");
  py::object d = torch.attr("device")("cuda", dev), f32 = torch.attr("float32");
  py::object p = priority.attr("detach")().attr("to")(d, f32).attr("contiguous")(), s = seq_len.attr("to")(d, f32).attr("contiguous")();
  const auto shp = p.attr("shape").cast<std::vector<int64_t>>();
  if (shp.size() != 2) throw std::runtime_error("aggregate_priority: priority must be [T, B]");
  py::object out = torch.attr("empty")(py::make_tuple(shp[1]), py::arg("dtype") = f32, py::arg("device") = d);
  auto ptr = [](const py::object& t) { return reinterpret_cast<float*>(t.attr("data_ptr")().cast<uintptr_t>()); };
  ck(hsad_aggregate_priority(ptr(p), ptr(s), (int)shp[0], (int)shp[1], eta, ptr(out), torch_stream(dev)));
  return on_gpu ? out : out.attr("cpu")();
}

class ThreadLoop;

// rela.R2D2Actor: configuration of an actor; the loop it is attached to counts its acts (R2D2Actor::numAct_ += batchsize per act())
class R2D2Actor {
 public:
  std::shared_ptr<BatchRunner> runner;
  int multi_step = 1, num_envs = 0, seq_len = 0, num_player = 1;
  float gamma = 0.99f, eta = 0.9f;
  std::shared_ptr<RNNPrioritizedReplay> replay;
  bool eval_only = false;
  std::shared_ptr<std::atomic<int64_t>> steps;      // steps of the loop that drives this actor (shared: outlives the loop and its Context)
  int per_step = 0;
  R2D2Actor(std::shared_ptr<BatchRunner> r, int multi_step_, int batchsize, float gamma_, float eta_, int seq_len_, int num_player_,
            std::shared_ptr<RNNPrioritizedReplay> rep)
      : runner(std::move(r)), multi_step(multi_step_), num_envs(batchsize), seq_len(seq_len_), num_player(num_player_), gamma(gamma_), eta(eta_),
        replay(std::move(rep)) {}
  R2D2Actor(std::shared_ptr<BatchRunner> r, int num_player_) : runner(std::move(r)), num_player(num_player_), eval_only(true) {}
  int64_t num_act() const { return steps ? steps->load() * per_step : 0; }
};

// rela.ThreadLoop: base of hanalearn.HanabiThreadLoop (bound as its parent like in the reference, rela/pybind.cc:60, cpp/pybind.cc:45)
class ThreadLoop {
 public:
  virtual ~ThreadLoop() = default;
  virtual void build() = 0;                 // (Context.start) create the device objects
  virtual bool step() = 0;                  // one lock-step iteration for all games; false = finished (eval loops)
  virtual bool finished() const = 0;
  virtual int device_id() const = 0;
  virtual bool try_absorb(ThreadLoop&) { return false; }
  virtual void validate() const {}          // (Context.push_env_thread) refuse what this face cannot run
  bool absorbed = false;                    // merged into another loop of the Context: that one steps its games
};

// a Python context manager entered for the lifetime of this object (GIL held)
struct PyScope {
  py::object cm;
  explicit PyScope(py::object c) : cm(std::move(c)) { cm.attr("__enter__")(); }
  ~PyScope() {
    try {
      cm.attr("__exit__")(py::none(), py::none(), py::none());
    } catch (...) {
    }
  }
};

// hanalearn.HanabiThreadLoop
class HanabiThreadLoop : public ThreadLoop {
 public:
  std::vector<std::vector<std::shared_ptr<R2D2Actor>>> groups;      // actor(s) of every merged thread
  std::vector<std::shared_ptr<HanabiVecEnv>> vec_envs;
  bool is_list, eval_mode;
  std::shared_ptr<BatchedEnv> env;
  hsad_actor* actor = nullptr;
  hipStream_t stream = nullptr;
  std::shared_ptr<std::atomic<int64_t>> steps = std::make_shared<std::atomic<int64_t>>(0);
  std::atomic<bool> done{false};      // read by Context::terminated on the driver's thread while the loop thread writes it
  bool built = false;
  // eval state: one acting net per seat (the same net for all seats = one pass over all rows)
  std::vector<std::shared_ptr<BatchRunner>> seats;
  bool same_model = true;
  std::vector<DevBuf> h_in, c_in, h_out, c_out, act_a, act_g;
  DevBuf joint;
  uint64_t counter = 0;
  // contract seats: the model's hidden state {h0, c0} [L, rows, H] per model, and the rollout stream as a torch stream (GIL to touch)
  std::vector<py::object> c_hid;
  py::object ext_stream;

  HanabiThreadLoop(std::vector<std::shared_ptr<R2D2Actor>> actors, std::shared_ptr<HanabiVecEnv> vec, bool eval, bool list)
      : is_list(list), eval_mode(eval) {
    if (actors.empty() || !vec || vec->envs.empty()) throw std::runtime_error("HanabiThreadLoop needs at least one actor and a non-empty HanabiVecEnv");
    groups.push_back(std::move(actors));
    vec_envs.push_back(std::move(vec));
  }
  ~HanabiThreadLoop() override {
    if (actor) hsad_actor_destroy(actor);
    if (ext_stream || !c_hid.empty()) {      // torch objects used on the rollout stream: released while it still exists
      py::gil_scoped_acquire gil;
      c_hid.clear();
      ext_stream = py::object();
    }
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
  }
  int device_id() const override { return groups[0][0]->runner->device; }
  bool finished() const override { return eval_mode && done.load(); }
  void validate() const override {
    if (eval_mode) return;
    for (const auto& g : groups)
      for (const auto& a : g)
        if (a->runner->contract)
          throw std::runtime_error(
              "HanabiThreadLoop: a training loop over a model behind the act / get_h0 contract (not the R2D2Net shape) runs on the Python face "
              "(hanabi_sad_amd.rela / hanabi_sad_amd.hanalearn, re-exported by the repository's rela / hanalearn packages); the compiled "
              "modules run such models in evaluation loops only");
  }
  std::pair<int, int> seed_range() const {
    int lo = vec_envs.front()->envs.front()->cfg.seed, hi = lo - 1;
    for (const auto& v : vec_envs) hi += (int)v->envs.size();
    return {lo, hi};
  }
  bool seeds_consecutive() const {
    int want = vec_envs.front()->envs.front()->cfg.seed;
    const EnvCfg& c0 = vec_envs.front()->envs.front()->cfg;
    for (const auto& v : vec_envs)
      for (const auto& e : v->envs) {
        if (e->cfg.seed != want++ || !e->cfg.same_but_seed(c0)) return false;
      }
    return true;
  }
  // Context merges loops that continue each other's seed range and share models, replay and configuration (create.py builds one loop per
  // thread -- eval.py one per GAME): one batched device loop, one launch per kernel, instead of one set of launches per loop
  bool try_absorb(ThreadLoop& other_) override {
    auto* o = dynamic_cast<HanabiThreadLoop*>(&other_);
    if (!o || built || o->built || o->absorbed || eval_mode != o->eval_mode || is_list != o->is_list) return false;
    const auto &a = groups[0], &b = o->groups[0];
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
      if (a[i]->runner != b[i]->runner || a[i]->replay != b[i]->replay || a[i]->multi_step != b[i]->multi_step || a[i]->gamma != b[i]->gamma ||
          a[i]->eta != b[i]->eta || a[i]->seq_len != b[i]->seq_len || a[i]->num_player != b[i]->num_player || a[i]->eval_only != b[i]->eval_only)
        return false;
    }
    if (!vec_envs[0]->envs[0]->cfg.same_but_seed(o->vec_envs[0]->envs[0]->cfg) || !seeds_consecutive() || !o->seeds_consecutive() ||
        o->seed_range().first != seed_range().second + 1)
      return false;
    for (auto& g : o->groups) groups.push_back(g);
    for (auto& v : o->vec_envs) vec_envs.push_back(v);
    o->absorbed = true;
    return true;
  }
  void build() override {
    if (built) return;
    built = true;
    if (!seeds_consecutive())
      throw std::runtime_error("HanabiVecEnv: the games of a vector env must differ only by seed = seed0 + index (what create.py:36-53 builds)");
    validate();
    const auto& a0 = groups[0];
    BatchRunner& run = *a0[0]->runner;
    const int dev = run.device;
    hipck(hipSetDevice(dev), "hipSetDevice");
    int G = 0;
    for (const auto& v : vec_envs) G += (int)v->envs.size();
    const EnvCfg& c0 = vec_envs[0]->envs[0]->cfg;
    env = std::make_shared<BatchedEnv>(G, c0, dev, false);
    int r = 0;
    for (const auto& v : vec_envs)
      for (const auto& e : v->envs) {
        e->batch = env;
        e->row = r++;
      }
    const int P = env->P;
    // the models acting in this loop: the training runner, or one per seat (cross-play when the runners differ, eval.py:43-46)
    std::vector<std::shared_ptr<BatchRunner>> runs{a0[0]->runner};
    if (eval_mode) {
      runs.clear();
      for (int p = 0; p < P; ++p) runs.push_back((is_list && (int)a0.size() == P) ? a0[p]->runner : a0[0]->runner);
    }
    BatchRunner* kernel_run = nullptr;      // the first seat on the kernels (its padded input row sizes the bf16 observation)
    bool any_contract = false;
    for (auto& s : runs) {
      if (s->device != dev) throw std::runtime_error("HanabiThreadLoop: the seats' models must share one device");
      if (s->contract) {
        any_contract = true;
        continue;
      }
      if (env->F != s->in_dim || env->A != s->num_action)
        throw std::runtime_error("HanabiThreadLoop: the model's in_dim / num_action do not match the env's feature_size / num_action");
      if (!kernel_run) kernel_run = s.get();
    }
    hipck(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
    // a contract model reads the float32 observation (as on the Python face): keep writing it next to the packed outputs
    if (kernel_run) env->enable_packed(hsad_r2d2_net_in_dim_padded(kernel_run->online), any_contract);
    // acts counted like R2D2Actor::numAct_: += its batchsize (its thread's games) per step
    for (size_t t = 0; t < groups.size(); ++t)
      for (auto& a : groups[t]) {
        a->steps = steps;
        a->per_step = (int)vec_envs[t]->envs.size();
      }
    if (!eval_mode) {
      const bool vdn = !is_list && a0[0]->num_player > 1;
      if (!a0[0]->replay) throw std::runtime_error("HanabiThreadLoop: a training loop needs actors with a replay buffer");
      a0[0]->replay->bind_schema(env->F, env->A, env->H, vdn ? P : 1, a0[0]->seq_len, dev);
      hsad_actor_config cfg{};
      cfg.vdn = vdn;
      cfg.multi_step = a0[0]->multi_step;
      cfg.seq_len = a0[0]->seq_len;
      cfg.hand_size = env->H;
      cfg.hid_dim = run.hid;
      cfg.gamma = a0[0]->gamma;
      cfg.eta = a0[0]->eta;
      cfg.seed = (uint64_t)G;
      hsad_actor_io io{env->legal.as<float>(), env->own.as<float>(), env->eps.as<float>(), env->reward.as<float>(), env->terminal.as<uint8_t>(),
                       env->priv_bits.as<uint64_t>(), env->legal_bits.as<uint64_t>(), env->own_bits.as<uint64_t>(), env->priv_bf16.p};
      ck(hsad_actor_create(env->h, run.online, run.target, a0[0]->replay->h, &cfg, &io, &actor));
      ck(hsad_actor_set_run_ahead(actor, 3));      // free-running, the host at most three steps ahead of the device
      return;
    }
    // evaluation: every seat acts greedily with ITS actor's model (cross-play when the runners differ, eval.py:43-46)
    seats = runs;
    same_model = true;
    for (auto& s : seats) same_model = same_model && s == seats[0];
    const size_t N = (size_t)G * P, nm = same_model ? 1 : P;
    h_in = std::vector<DevBuf>(nm);
    c_in = std::vector<DevBuf>(nm);
    h_out = std::vector<DevBuf>(nm);
    c_out = std::vector<DevBuf>(nm);
    act_a = std::vector<DevBuf>(nm);
    act_g = std::vector<DevBuf>(nm);
    c_hid = std::vector<py::object>(nm);
    py::object torch = py::module_::import("torch");
    py::object tdev = torch.attr("device")("cuda", dev);
    for (size_t m = 0; m < nm; ++m) {
      const BatchRunner& rr = *seats[m];
      const size_t hb = rr.contract ? 0 : (size_t)rr.nl * N * rr.hid * 4;
      h_in[m].alloc(hb);
      c_in[m].alloc(hb);
      h_out[m].alloc(hb);
      c_out[m].alloc(hb);
      act_a[m].alloc(N * 8);
      act_g[m].alloc(N * 8);
      if (!rr.contract) continue;
      // ContractAgent.get_h0 of the Python face (hanabi_sad_amd/rela.py): float32 on the device, [L, rows, H]
      const int64_t rows = same_model ? (int64_t)N : G;
      py::dict h0;
      {
        PyScope ng(torch.attr("no_grad")());
        h0 = rr.impl.attr("get_h0")(rows);
      }
      py::dict hid;
      for (auto kv : h0) {
        py::object v = kv.second.attr("to")(tdev).attr("float")();
        const auto shp = BatchRunner::shape_of(v);
        if (shp.size() == 3 && shp[1] != rows && shp[0] == rows) v = v.attr("transpose")(0, 1);
        hid[kv.first] = v.attr("contiguous")();
      }
      c_hid[m] = hid;
    }
    joint.alloc(N * 8);
    if (any_contract) {
      ext_stream = torch.attr("cuda").attr("ExternalStream")(reinterpret_cast<uintptr_t>(stream), py::arg("device") = tdev);
      torch.attr("cuda").attr("current_stream")(tdev).attr("synchronize")();      // the hidden states exist before the first act
    }
    ck(hsad_env_reset(env->h, stream));
  }
  // one greedy act of contract model m on the rollout stream, as rela.ContractAgent.act of the Python face shapes it: [1, rows, ...] inputs,
  // h0 / c0 [1, rows, L, H]; its greedy actions land in act_g[m] (all rows, or seat m's column in cross-play)
  void contract_act(size_t m) {
    BatchRunner& rr = *seats[m];
    const int G = env->G, P = env->P, F = env->F, A = env->A;
    const int64_t R = same_model ? (int64_t)G * P : G;
    const hipStream_t s = stream;
    py::gil_scoped_acquire gil;      // only around the model call
    try {
      auto lk = rr.lock_with_gil();
      py::object torch = py::module_::import("torch");
      py::object tdev = torch.attr("device")("cuda", env->device);
      PyScope on_stream(torch.attr("cuda").attr("stream")(ext_stream));
      PyScope ng(torch.attr("no_grad")());
      auto empty = [&](std::vector<int64_t> shape) {
        return torch.attr("empty")(py::cast(shape), py::arg("dtype") = torch.attr("float32"), py::arg("device") = tdev);
      };
      auto ptr = [](const py::object& t) { return reinterpret_cast<void*>(t.attr("data_ptr")().cast<uintptr_t>()); };
      py::object priv = empty({1, R, F}), legal = empty({1, R, A});
      if (same_model) {
        hipck(hipMemcpyAsync(ptr(priv), env->priv_s.p, (size_t)R * F * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
        hipck(hipMemcpyAsync(ptr(legal), env->legal.p, (size_t)R * A * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
      } else {      // seat m's rows of the [G, P, .] outputs
        hipck(hipMemcpy2DAsync(ptr(priv), (size_t)F * 4, env->priv_s.as<float>() + (size_t)m * F, (size_t)P * F * 4, (size_t)F * 4, G,
                               hipMemcpyDeviceToDevice, s),
              "hipMemcpy2DAsync");
        hipck(hipMemcpy2DAsync(ptr(legal), (size_t)A * 4, env->legal.as<float>() + (size_t)m * A, (size_t)P * A * 4, (size_t)A * 4, G,
                               hipMemcpyDeviceToDevice, s),
              "hipMemcpy2DAsync");
      }
      py::dict d;
      d["priv_s"] = priv;
      d["legal_move"] = legal;
      d["eps"] = torch.attr("zeros")(py::make_tuple(1, R), py::arg("dtype") = torch.attr("float32"), py::arg("device") = tdev);
      py::dict hid = c_hid[m];
      for (const char* k : {"h0", "c0"}) {
        py::object h = hid[k];
        h.attr("record_stream")(ext_stream);
        d[k] = h.attr("transpose")(0, 1).attr("unsqueeze")(0).attr("contiguous")();
      }
      py::dict reply = rr.impl.attr("act")(d);
      py::dict nh;
      for (const char* k : {"h0", "c0"}) {
        const auto like = BatchRunner::shape_of(hid[k]);
        nh[k] = reply[k].attr("to")(tdev).attr("reshape")(like[1], like[0], like[2]).attr("transpose")(0, 1).attr("contiguous")();
      }
      c_hid[m] = nh;
      py::object g = reply["greedy_a"].attr("to")(tdev).attr("reshape")(-1).attr("long")().attr("contiguous")();
      if (g.attr("numel")().cast<int64_t>() != R)
        throw std::runtime_error("the model's act returned " + std::to_string(g.attr("numel")().cast<int64_t>()) + " greedy actions for " +
                                 std::to_string(R) + " rows");
      if (same_model)
        hipck(hipMemcpyAsync(act_g[m].p, ptr(g), (size_t)R * 8, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync");
      else
        hipck(hipMemcpy2DAsync(act_g[m].as<int64_t>() + m, (size_t)P * 8, ptr(g), 8, 8, G, hipMemcpyDeviceToDevice, s), "hipMemcpy2DAsync");
    } catch (py::error_already_set& e) {
      throw std::runtime_error(std::string("BatchRunner: the model's act raised: ") + e.what());
    }
  }
  bool step() override {
    if (absorbed) return !finished();
    hipck(hipSetDevice(device_id()), "hipSetDevice");
    if (!eval_mode) {
      std::lock_guard<std::mutex> g(groups[0][0]->runner->mu);
      ck(hsad_actor_step(actor, stream));
      steps->fetch_add(1);
      return true;
    }
    if (done.load()) return false;
    const auto q = env->read_query(stream);
    bool all = true;
    for (int g = 0; g < env->G; ++g) all = all && q[(size_t)g * HSAD_QUERY_WORDS + HSAD_Q_TERMINATED] != 0;
    if (all) {
      int32_t n = 0, fg = 0, fc = 0;
      ck(hsad_env_error_count(env->h, &n, &fg, &fc));      // drain the "step on a finished game" notes of the last iterations
      done.store(true);
      return false;
    }
    const int N = env->G * env->P, P = env->P;
    for (size_t m = 0; m < h_in.size(); ++m) {
      BatchRunner& rr = *seats[m];
      if (rr.contract) {
        contract_act(m);
        continue;
      }
      std::lock_guard<std::mutex> g(rr.mu);
      ck(hsad_r2d2_act(rr.online, nullptr, N, nullptr, env->priv_bf16.p, env->legal.as<float>(), nullptr, h_in[m].as<float>(), c_in[m].as<float>(), nullptr,
                       (uint64_t)env->G, counter, act_a[m].as<int64_t>(), act_g[m].as<int64_t>(), h_out[m].as<float>(), c_out[m].as<float>(), nullptr,
                       nullptr, nullptr, stream));
      std::swap(h_in[m].p, h_out[m].p);
      std::swap(c_in[m].p, c_out[m].p);
    }
    ++counter;
    const int64_t* a = act_g[0].as<int64_t>();
    if (!same_model) {      // seat p's column of the joint action comes from model p (rows are (game, player) pairs)
      for (int p = 0; p < P; ++p)
        hipck(hipMemcpy2DAsync(joint.as<int64_t>() + p, (size_t)P * 8, act_g[p].as<int64_t>() + p, (size_t)P * 8, 8, env->G, hipMemcpyDeviceToDevice, stream),
              "hipMemcpy2DAsync");
      a = joint.as<int64_t>();
    }
    ck(hsad_env_step(env->h, a, a, stream));      // (finished games: left untouched by the library, noted, drained above)
    steps->fetch_add(1);
    return true;
  }
  void check_errors() {
    int32_t n = 0, g = 0, c = 0;
    ck(hsad_env_error_count(env->h, &n, &g, &c));
    if (n && !eval_mode) throw std::runtime_error("HanabiEnv: " + std::to_string(n) + " games hit an API-contract error (first: game " + std::to_string(g) + ")");
  }
};

// ---- rela.Context: ONE thread that advances every attached loop, free-running (rela/context.h:14-99) ----
class Context {
 public:
  std::vector<std::shared_ptr<ThreadLoop>> loops;
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  bool started = false, paused = false, parked = false, stop = false, finished_all = false;
  std::string error;
  ~Context() { terminate(); }
  int push_env_thread(std::shared_ptr<ThreadLoop> lp) {
    if (started) throw std::runtime_error("Context.push_env_thread after start()");
    lp->validate();
    loops.push_back(std::move(lp));
    return (int)loops.size();
  }
  void start() {
    if (started) return;
    // merge compatible loops, build the device objects (allocations, kernels of the first reset) on the caller's thread
    for (size_t i = 0; i < loops.size(); ++i) {
      if (loops[i]->absorbed) continue;
      for (size_t j = i + 1; j < loops.size(); ++j)
        if (!loops[j]->absorbed) loops[i]->try_absorb(*loops[j]);
    }
    for (auto& lp : loops)
      if (!lp->absorbed) lp->build();
    started = true;
    py::gil_scoped_release nogil;
    th = std::thread([this] { run(); });
  }
  void run() {
    try {
      for (;;) {
        {
          std::unique_lock<std::mutex> g(mu);
          if (stop) break;
          if (paused) {
            parked = true;
            cv.notify_all();
            cv.wait(g, [this] { return !paused || stop; });
            parked = false;
            continue;
          }
        }
        bool busy = false;
        for (auto& lp : loops)
          if (!lp->absorbed && !lp->finished()) busy = lp->step() || busy;
        if (!busy) break;
      }
    } catch (const std::exception& e) {
      std::lock_guard<std::mutex> g(mu);
      error = e.what();
    }
    std::lock_guard<std::mutex> g(mu);
    finished_all = true;
    parked = true;
    cv.notify_all();
  }
  // The loop thread takes the GIL around the calls of contract models: whatever waits for it (its lock, its parking, its end) waits
  // without the GIL.  The loop thread never takes the GIL while it holds `mu`.
  void check() {
    std::string e;
    {
      py::gil_scoped_release nogil;
      std::lock_guard<std::mutex> g(mu);
      e.swap(error);
    }
    if (!e.empty()) throw std::runtime_error("Context loop thread: " + e);
  }
  void pause() {      // blocks until the loop thread is parked between two steps (rela/context.h:52-60)
    check();
    py::gil_scoped_release nogil;
    std::unique_lock<std::mutex> g(mu);
    paused = true;
    if (started) cv.wait(g, [this] { return parked || finished_all; });
  }
  void resume() {
    check();
    std::lock_guard<std::mutex> g(mu);
    paused = false;
    cv.notify_all();
  }
  void terminate() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
      paused = false;
      cv.notify_all();
    }
    if (!th.joinable()) return;
    if (PyGILState_Check()) {      // (the destructor may run without the GIL)
      py::gil_scoped_release nogil;
      th.join();
    } else {
      th.join();
    }
  }
  bool terminated() {
    check();
    py::gil_scoped_release nogil;
    std::lock_guard<std::mutex> g(mu);
    if (!started) return false;
    if (finished_all) return true;
    for (auto& lp : loops)
      if (!lp->absorbed && !lp->finished()) return false;
    return true;
  }
};

}  // namespace hsadpy
