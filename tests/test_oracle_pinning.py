"""Pin the CPU restatement (oracle/restate.py) against the golden vectors generated from the
reference (tests/golden/, oracle/gen_goldens.py) and against the reference's own classes on fresh shapes (their results
recorded in tests/golden/reference/, golden_io.recorded).  CPU only."""
import numpy as np
import pytest
import torch

from oracle import restate as O
from oracle import ref_shim
from golden_io import Golden, MODEL_CASES, recorded

RTOL, ATOL = 2e-5, 2e-6


def close(a, b, rtol=RTOL, atol=ATOL, what=""):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    tol = (torch.as_tensor(atol).double().reshape(-1) if torch.is_tensor(atol) else atol) + rtol * b.abs()
    assert bool((err <= tol).all()), f"{what}: max err {err.max().item():.3e} (ref max {b.abs().max().item():.3e})"


def shadow_atol(grad, grad_norm, lr, steps, default):
    """Biases whose only path to the loss runs through a BatchNorm with nothing but linear maps in
    between (MLP.layer_1.bias, reference modules.py:145-146; in DirectPred also encoders.*.layer_out.bias
    and fusion_block.bias, because every head starts Linear->BN) have a true gradient of exactly 0: what
    any implementation computes for them is rounding noise (~1e-9).  Adam turns noise of ANY magnitude
    into a step of up to lr, so those entries are implementation-defined (the reference itself differs
    between 1 and 8 CPU threads) and cannot affect any loss.  Detected from the golden gradient."""
    if grad is None:
        return default
    # element-wise: a hidden unit whose pre-activations share one sign over the batch makes LeakyReLU
    # linear there, so even Encoder/Decoder biases can have single exactly-zero-gradient elements.
    noise = grad.abs() < 1e-6 * float(grad_norm)
    # opposite-sign noise: up to 2*lr apart per step
    return torch.where(noise, torch.tensor(2.1 * lr * steps), torch.tensor(float(default)))


@pytest.mark.parametrize("case", MODEL_CASES)
def test_state_manifest_matches_reference_keys(case):
    g = Golden(case)
    man = O.state_manifest(g.spec)
    st0 = g.state0()
    assert set(man) == set(st0)
    for k, shp in man.items():
        assert tuple(st0[k].shape) == shp, k


def golden_opt(g, s):
    """Adam state the reference held after step s (s = -1 -> fresh optimiser)."""
    if s < 0:
        return {}
    return {"t": s + 1, "m": g.exp(s, "m"), "v": g.exp(s, "v")}


@pytest.mark.parametrize("case", MODEL_CASES)
def test_each_train_step_matches_reference(case):
    """Per-step parity: step s starts from the reference's state after step s-1."""
    g = Golden(case)
    spec = g.spec
    for s in range(g.n_steps):
        st_in = g.state0() if s == 0 else g.exp(s - 1, "state")
        st, opt, info = O.train_step(spec, st_in, golden_opt(g, s - 1), g.batch(s), g.draws(s), g.lr)
        for k, v in g.exp(s, "loss").items():
            close(info["losses"][k], v, what=f"{case} step{s} loss {k}")
        exp_grads = g.exp(s, "grad")
        assert set(exp_grads) == set(info["grads"]), (set(exp_grads) ^ set(info["grads"]))
        for k, v in exp_grads.items():
            close(info["grads"][k], v, rtol=1e-4, atol=1e-6, what=f"{case} step{s} grad {k}")
        gn = g.get(f"exp/{s}/grad_norm")
        close(info["grad_norm"], gn, what="grad_norm")
        for k, v in g.exp(s, "state").items():
            close(st[k], v, rtol=1e-4, atol=shadow_atol(exp_grads.get(k), gn, g.lr, 1, 2e-6),
                  what=f"{case} step{s} state {k}")
        for k, v in g.exp(s, "m").items():
            close(opt["m"][k], v, rtol=1e-4, atol=1e-7, what=f"{case} step{s} m {k}")
        for k, v in g.exp(s, "v").items():
            close(opt["v"][k], v, rtol=1e-4, atol=1e-9, what=f"{case} step{s} v {k}")


@pytest.mark.parametrize("case", MODEL_CASES)
def test_free_running_loss_trajectory(case):
    """Free-running K-step trajectory: every named loss stays within 1e-4 relative of the reference."""
    g = Golden(case)
    spec, st, opt = g.spec, g.state0(), {}
    for s in range(g.n_steps):
        st, opt, info = O.train_step(spec, st, opt, g.batch(s), g.draws(s), g.lr)
        for k, v in g.exp(s, "loss").items():
            close(info["losses"][k], v, rtol=1e-4, atol=1e-6, what=f"{case} free-run step{s} loss {k}")


@pytest.mark.parametrize("case", MODEL_CASES)
def test_validation_and_predict_match_reference(case):
    g = Golden(case)
    spec = g.spec
    st = g.exp(g.n_steps - 1, "state")
    draws = g.sub("draws/val")
    losses, _ = O.eval_losses(spec, st, g.batch(0), draws)
    for k, v in g.sub("exp/val/loss").items():
        close(losses[k], v, what=f"{case} val {k}")
    if spec.model != "MultiTripletNetwork":
        cohort = g.sub("cohort")
        xs = [cohort[name] for name, _ in spec.layers]
        svae = spec.is_vae
        emb, _ = O.predict_outputs(spec, st, xs, g.get("draws/transform/eps") if svae else None)
        close(emb, g.get("exp/transform"), rtol=1e-4, atol=1e-5, what="transform")
        _, outs = O.predict_outputs(spec, st, xs, g.get("draws/predict/eps") if svae else None)
        for k, v in g.sub("exp/predict").items():
            close(outs[k], v, rtol=1e-4, atol=1e-5, what=f"predict {k}")


def test_function_goldens():
    g = Golden("functions")
    for tag in ("plain", "with_nan", "all_censored", "none_valid", "single_valid", "large_batch"):
        c = g.sub(f"cox/{tag}")
        o = c["outputs"].clone().requires_grad_(True)
        l = O.cox_ph(o, c["durations"], c["events"])
        close(l, c["loss"], what=f"cox {tag}")
        gr = torch.autograd.grad(l, o)[0] if l.requires_grad else torch.zeros_like(o)
        close(gr, c["grad"], rtol=1e-4, atol=1e-7, what=f"cox grad {tag}")
    for tag, fn in (("mse/plain", O.mse_masked), ("mse/with_nan", O.mse_masked), ("mse/all_missing", O.mse_masked),
                    ("ce/plain", O.ce_masked), ("ce/with_missing", O.ce_masked), ("ce/all_missing", O.ce_masked)):
        c = g.sub(tag)
        yh = c["yhat"].clone().requires_grad_(True)
        l = fn(yh, c["y"])
        close(l, c["loss"], what=tag)
        gr = torch.autograd.grad(l, yh)[0] if l.requires_grad else torch.zeros_like(yh)
        close(gr, c["grad"], rtol=1e-4, atol=1e-7, what=tag + " grad")
    t = g.sub("triplet")
    a, p, n = (t[k].clone().requires_grad_(True) for k in ("a", "p", "n"))
    l = O.triplet(a, p, n)
    close(l, t["loss"], what="triplet")
    ga, gp, gn = torch.autograd.grad(l, (a, p, n))
    close(ga, t["grad_a"]); close(gp, t["grad_p"]); close(gn, t["grad_n"])
    m = g.sub("mmd")
    z, xh = m["z"].clone().requires_grad_(True), m["xhat"].clone().requires_grad_(True)
    l = O.mmd_loss(z, xh, m["x"], m["prior"])
    close(l, m["loss"], what="mmd")
    gz, gx = torch.autograd.grad(l, (z, xh))
    close(gz, m["grad_z"], rtol=1e-4, atol=1e-8); close(gx, m["grad_xhat"], rtol=1e-4, atol=1e-8)
    close(O.gaussian_kernel(m["z"], m["z"]), m["kernel_zz"], what="kernel")
    r = g.sub("reparam")
    close(r["mean"] + r["log_var"] * r["eps"], r["z"], what="reparam")
    tot = g.sub("total")
    spec = O.Spec("DirectPred", [("gex", 16)], 4, 0.5, 4, [("y", "numerical", 1), ("c", "categorical", 3)])
    st = {"log_vars.y": torch.tensor([0.3]), "log_vars.c": torch.tensor([-0.2])}
    close(O.total_loss(spec, st, {"y": tot["l1"], "c": tot["l2"]}, True), tot["weighted"], what="weighted total")
    close(O.total_loss(spec, st, {"y": tot["l1"]}, True), tot["single"], what="single-term total")


def _reference_steps(spec, dat, ann, vt, batches, **kw):
    """The reference's own model class through ref_capture.reference_train_steps from perturbed_state(seed=3): per step the loss,
    the draws, the gradients, the clip norm and the state after the step."""
    from oracle import ref_capture
    from oracle.gen_goldens import perturbed_state
    R = ref_shim.load()
    ds = ref_capture.make_dataset(R, dat, ann, vt)
    cfg = {"latent_dim": spec.latent_dim, "hidden_dim_factor": spec.hidden_dim_factor, "lr": 3e-3,
           "supervisor_hidden_dim": spec.supervisor_hidden_dim, "epochs": 1, "batch_size": 6}
    model = ref_capture.build_reference_model(R, spec, ds, cfg)
    model.load_state_dict(perturbed_state(spec, seed=3))
    recs = ref_capture.reference_train_steps(R, spec, model, batches, 3e-3, **kw)
    return [{"total": r.total, "draws": r.draws, "grads": r.grads, "grad_norm": r.grad_norm, "state": r.state} for r in recs]


def test_live_reference_step_matches_oracle():
    """Fresh shapes/seeds (not the committed goldens): reference vs restatement, one step each model (the reference's side recorded
    in tests/golden/reference/live_step_*.npz)."""
    from types import SimpleNamespace
    from oracle.gen_goldens import make_cohort, make_batches, perturbed_state
    specs = [
        O.Spec("DirectPred", [("a", 33), ("b", 21)], 5, 0.4, 3, [("c", "categorical", 4), ("y", "numerical", 1)]),
        O.Spec("supervised_vae", [("a", 30), ("b", 18)], 6, 0.3, 3, [("y", "numerical", 1)]),
        O.Spec("MultiTripletNetwork", [("a", 20), ("b", 26)], 4, 0.5, 3, [("c", "categorical", 3)]),
        O.Spec("CrossModalPred", [("a", 30), ("b", 18), ("d", 22)], 6, 0.3, 3, [("c", "categorical", 3)],
               input_layers=["b"], output_layers=["a", "d"]),
        # unsupervised runs (reference __main__.py:997 accepts these classes without target variables): mmd_loss only
        O.Spec("supervised_vae", [("a", 30), ("b", 18)], 6, 0.3, 3, []),
        O.Spec("CrossModalPred", [("a", 30), ("b", 18), ("d", 22)], 6, 0.3, 3, [], input_layers=["a", "b"],
               output_layers=["d", "a"]),
    ]
    for i, spec in enumerate(specs):
        dat, ann, vt = make_cohort(spec, 30, seed=9, missing=False)
        st0 = perturbed_state(spec, seed=3)
        batches = make_batches(spec, dat, ann, 6, 2, seed=4, missing=False)
        recs = [SimpleNamespace(**r) for r in
                recorded(f"live_step_{i}_{spec.model}", lambda: _reference_steps(spec, dat, ann, vt, batches))]
        st, opt = st0, {}
        for si, (b, r) in enumerate(zip(batches, recs)):
            st, opt, info = O.train_step(spec, st, opt, b, r.draws, 3e-3)
            close(info["losses"]["total"], r.total, rtol=1e-4, what=spec.model + " total")
            if si == 0:
                for k, v in r.state.items():
                    close(st[k], v, rtol=1e-4, atol=shadow_atol(r.grads.get(k), r.grad_norm, 3e-3, 1, 2e-6),
                          what=f"{spec.model} {k}")


@pytest.mark.parametrize("freeze", [{"encoders": True, "supervisors": False}, {"encoders": False, "supervisors": True}])
def test_live_reference_finetune_step_matches_oracle(freeze):
    """FineTuner steps (reference main.py:530-539, :562-566, :591-600): frozen parameter groups, Adam over the
    trainable ones, NO gradient clipping -- reference (recorded in tests/golden/reference/live_finetune_*.npz) vs the
    restatement's train_step(clip=False, frozen=...)."""
    from types import SimpleNamespace
    from oracle.gen_goldens import make_cohort, make_batches, perturbed_state
    frozen = tuple(p for p, on in (("encoders.", freeze["encoders"]), ("MLPs.", freeze["supervisors"])) if on)
    tag = "enc_frozen" if freeze["encoders"] else "sup_frozen"
    for spec in (O.Spec("DirectPred", [("a", 33), ("b", 21)], 5, 0.4, 3, [("c", "categorical", 4), ("y", "numerical", 1)]),
                 O.Spec("supervised_vae", [("a", 30), ("b", 18)], 6, 0.3, 3, [("y", "numerical", 1)])):
        dat, ann, vt = make_cohort(spec, 30, seed=9, missing=False)
        st0 = perturbed_state(spec, seed=3)
        batches = make_batches(spec, dat, ann, 6, 2, seed=4, missing=False)
        recs = [SimpleNamespace(**r) for r in recorded(f"live_finetune_{tag}_{spec.model}",
                                                       lambda: _reference_steps(spec, dat, ann, vt, batches, clip=False, freeze=freeze))]
        st, opt = st0, {}
        for si, (b, r) in enumerate(zip(batches, recs)):
            st, opt, info = O.train_step(spec, st, opt, b, r.draws, 3e-3, clip=False, frozen=frozen)
            close(info["losses"]["total"], r.total, rtol=1e-4, what=spec.model + " total")
            assert set(info["grads"]) == set(r.grads), set(info["grads"]) ^ set(r.grads)
            if si == 0:
                for k, v in r.state.items():
                    if k.startswith(frozen) and not O.is_buffer(k):
                        assert torch.equal(st[k], st0[k]) and torch.equal(v, st0[k]), k       # frozen: bit-identical
                    else:
                        close(st[k], v, rtol=1e-4, atol=shadow_atol(r.grads.get(k), r.grad_norm, 3e-3, 1, 2e-6),
                              what=f"{spec.model} {k}")


@pytest.mark.parametrize("model", ["DirectPred", "supervised_vae"])
@pytest.mark.parametrize("freeze", ["enc_frozen", "sup_frozen"])
def test_finetune_step_fixture_pins_the_oracles_frozen_mode(model, freeze):
    """The same pin as the live test above, from the committed fixture (tests/golden/finetune_step.npz, generated from the
    reference's own classes): it travels to the GPU box, where the engine's frozen plans are checked against it."""
    from golden_io import FinetuneGolden
    G = FinetuneGolden(model)
    spec, frozen = G.spec, FinetuneGolden.FREEZES[freeze]
    st0 = G.state0()
    st, opt = st0, {}
    for s in range(2):
        exp = G.step(freeze, s)
        st, opt, info = O.train_step(spec, st, opt, G.batch(s), exp["draws"], G.lr, clip=False, frozen=frozen)
        close(info["losses"]["total"], exp["total"], rtol=1e-5, what=f"{model} {freeze} total step {s}")
        assert set(info["grads"]) == set(exp["grads"]), set(info["grads"]) ^ set(exp["grads"])
        close(info["grad_norm"], exp["grad_norm"], rtol=1e-4, what="grad norm")
        for k, v in exp["grads"].items():        # per tensor in norm (the MMD term's cancellations make single entries of small
            d = (info["grads"][k].double() - v.double()).norm() / max(float(v.double().norm()), 1e-30)     # tensors reduction-order noise)
            if float(v.double().norm()) > 1e-6 * float(exp["grad_norm"]):      # else: a true-zero gradient (a bias in front of a BatchNorm), noise
                assert float(d) <= 5e-3, (k, float(d))
        for k, v in exp["state"].items():
            if k.startswith(frozen) and not O.is_buffer(k):
                assert torch.equal(st[k], st0[k]) and torch.equal(v, st0[k]), k       # frozen: bit-identical, in the reference too
            elif s == 0:
                close(st[k], v, rtol=1e-4, atol=shadow_atol(exp["grads"].get(k), exp["grad_norm"], G.lr, 1, 2e-6), what=f"{model} {k}")


def finetune_loop_check(G, per_unit, results, best, final, lr_tol=1.0):
    """Shared by the CPU pin (oracle) and the GPU test (engine): the outcome of run_experiments against tests/golden/finetune_loop.npz.
    Tolerances: the biases in front of a BatchNorm have a true gradient of exactly 0, every implementation computes rounding noise
    for them and Adam turns it into +-lr steps; train-mode BatchNorm cancels them, eval-mode BatchNorm
    (validation) lags behind by its running mean, so validation losses agree to a few lr (6e-3 at lr 1e-2 here) -- while the golden's
    early-stopping decisions have margins of 4e-3 (lr 1e-2) or cannot change the outcome (lr 2e-3)."""
    for unit, (val, stopped) in per_unit.items():
        gv, gs, _ = G.unit(unit)
        assert stopped == gs, (unit, stopped, gs)
        close(val, gv, rtol=1e-2 * lr_tol, what=f"unit {unit} val_loss")
    assert {G.unit(u)[1] for u in per_unit} == {0, 3}                 # fits that stop early and fits that never do
    assert [r["epochs"] for r in results] == [r["epochs"] for r in G.results]
    assert [r["freeze"] for r in results] == [r["freeze"] for r in G.results]
    assert [r["learning_rate"] for r in results] == [r["learning_rate"] for r in G.results]
    for a, b in zip(results, G.results):
        close(a["average_val_loss"], b["average_val_loss"], rtol=1e-2 * lr_tol, what="average_val_loss")
    assert best["learning_rate"] == G.best["learning_rate"] and best["freeze"] == G.best["freeze"] and best["epochs"] == G.best["epochs"] > 0
    gfinal, last = G.sub("state_final"), G.sub("state_last")
    walk = 4.0 * G.lrs[-1] * (G.max_epoch * 3 + 6) ** 0.5            # a +-lr random walk over the last fit's and the final fit's steps
    for k, v in gfinal.items():
        got = torch.as_tensor(final[k]).detach().cpu()
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(v), k
        elif k.endswith("layer_1.bias") or k.endswith("layer_out.bias") or k == "fusion_block.bias" or k.endswith("running_mean"):
            # (the running means track the pre-BatchNorm activations, which carry those biases)
            close(got, v, rtol=0.0, atol=walk, what=f"final {k} (zero-gradient bias: noise walk)")
        else:
            close(got, v, rtol=2e-2, atol=3e-3, what=f"final {k}")
    return gfinal, last


def test_finetune_loop_fixture_pins_the_restated_run_experiments():
    """oracle/loop.py::fine_tune_reference against the reference's own DirectPred driven through FineTuner.run_experiments
    (tests/golden/finetune_loop.npz): every fit's final validation loss and stopped epoch, the results table, the best
    configuration, the final model continued from the LAST fit with the best configuration's freeze flags."""
    from golden_io import FinetuneLoopGolden
    from oracle import loop
    G = FinetuneLoopGolden()
    final, best, results, per_unit = loop.fine_tune_reference(
        G.spec, G.sub("state0"), G.sub("dat"), G.sub("ann"), G.n, folds=G.folds, batch_size=G.B, learning_rates=G.lrs,
        freeze_configs=G.cfgs, max_epoch=G.max_epoch, perms_fn=G.perms_fn, draws_fn=G.draws_fn)
    gfinal, last = finetune_loop_check(G, per_unit, results, best, final)
    # frozen in the golden's final fit (supervisors): bit-identical to the last cross-validation model, in the reference itself
    assert G.best["freeze"]["supervisors"]
    for k in last:
        if k.startswith("MLPs.") and not O.is_buffer(k):
            assert torch.equal(gfinal[k], last[k]), k


# ---- one HPO trial's loop (oracle/loop.py) vs the reference model driven through the same schedule ---------------
def _loop_golden(name="directpred"):
    import json
    import os
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"trial_loop_{name}.npz"))
    d = json.loads(str(z["spec_json"]))
    d["layers"] = [tuple(x) for x in d["layers"]]
    d["variables"] = [tuple(x) for x in d["variables"]]
    sub = lambda p: {k[len(p):]: torch.from_numpy(np.array(z[k])) for k in z.keys() if k.startswith(p)}
    return z, O.Spec(**d), sub


def loop_golden_inputs(name="directpred"):
    z, spec, sub = _loop_golden(name)
    epochs, B = int(z["epochs"]), int(z["batch_size"])
    perms = [torch.from_numpy(z[f"perm/{e}"]) for e in range(epochs)]
    G = dict(z=z, spec=spec, sub=sub, epochs=epochs, B=B, lr=float(z["lr"]), perms=perms, st0=sub("state0/"), dat=sub("dat/"),
             ann=sub("ann/"), train_idx=torch.from_numpy(z["train_idx"]), val_idx=torch.from_numpy(z["val_idx"]),
             draws=lambda e, b: sub(f"draws/{e}/{b}/"), val_draws=None, batch_fn=None, val_batch_fn=None)
    if spec.is_vae:                       # eps / priors of the validation batches (epoch == epochs: the final trainer.validate)
        G["val_draws"] = lambda e, bi: sub(f"vdraws/{e}/{bi}/")
    if spec.model == "MultiTripletNetwork":
        from oracle import loop
        valid = torch.from_numpy(z["valid_indices"])
        G["valid"] = valid
        G["trip"] = lambda e, b: (torch.from_numpy(z[f"trip/{e}/{b}/pos"]), torch.from_numpy(z[f"trip/{e}/{b}/neg"]))
        G["vtrip"] = lambda e, bi: (torch.from_numpy(z[f"vtrip/{e}/{bi}/pos"]), torch.from_numpy(z[f"vtrip/{e}/{bi}/neg"]))
        G["batch_fn"] = lambda e, b, rows: loop.triplet_batch_of(spec, G["dat"], G["ann"], valid[rows], *G["trip"](e, b))
        G["val_batch_fn"] = lambda e, bi, rows: loop.triplet_batch_of(spec, G["dat"], G["ann"], valid[rows], *G["vtrip"](e, bi))
    return G


def loop_golden_expected(G):
    """Per-epoch means of what the reference logged, reduced as Lightning reduces on_epoch values (batch-size weighted)."""
    z, nb = G["z"], G["train_idx"].numel() // G["B"]
    hist = []
    for e in range(G["epochs"]):
        names = sorted({k.split("/")[3] for k in z.keys() if k.startswith(f"step/{e}/0/")})
        rec = {n: float(np.mean([float(z[f"step/{e}/{b}/{n}"]) for b in range(nb)])) for n in names}
        nv = len([k for k in z.keys() if k.startswith(f"val/{e}/") and k.endswith("/n")])
        w = [int(z[f"val/{e}/{bi}/n"]) for bi in range(nv)]
        rec["val_loss"] = float(np.sum([float(z[f"val/{e}/{bi}/val_loss"]) * w[bi] for bi in range(nv)]) / np.sum(w))
        hist.append(rec)
    return hist


def test_trial_loop_restatement_matches_reference_golden():
    """oracle/loop.py's fit_reference (the restated objective(): reference main.py:228-333) against the trajectory the
    reference's own DirectPred produced under the same shuffles and dropout masks: every logged value's epoch mean, the
    validation loss of every epoch, the final state."""
    from oracle import loop
    G = loop_golden_inputs()
    out = loop.fit_reference(G["spec"], G["st0"], G["dat"], G["ann"], G["train_idx"], G["val_idx"], batch_size=G["B"],
                             epochs=G["epochs"], lr=G["lr"], patience=0, perms=G["perms"], draws_fn=G["draws"])
    exp = loop_golden_expected(G)
    assert len(out["history"]) == G["epochs"] == len(exp) and out["stopped_epoch"] == 0 and out["epochs"] == G["epochs"]
    for e, (got, want) in enumerate(zip(out["history"], exp)):
        assert set(got) == set(want), (set(got) ^ set(want))          # the reference logs its losses under these names
        for k in want:
            # Free-running over 6 steps per epoch.  The validation loss is the looser one: in eval mode BatchNorm no longer
            # cancels the biases in front of it, and those biases take implementation-defined +-lr steps (their true
            # gradient is zero) -- the reference at 1 vs 8 threads differs by as much.
            close(got[k], want[k], rtol=1e-3 if k == "val_loss" else 2e-4, atol=2e-6, what=f"epoch {e} {k}")
        # ... so validate() itself is pinned tightly from the REFERENCE's weights at the end of this epoch
        v = loop.validate(G["spec"], G["sub"](f"state_epoch/{e}/"), G["dat"], G["ann"], G["val_idx"], G["B"])
        close(v, want["val_loss"], rtol=1e-5, what=f"epoch {e} validation from the reference's state")
    assert out["val_loss"] == out["history"][-1]["val_loss"]          # trainer.validate after fit: same weights, same batches
    final = G["sub"]("state_final/")
    for k, v in final.items():
        if k.endswith("num_batches_tracked"):
            assert int(out["state"][k]) == int(v), k
        elif k.endswith("running_var"):
            # (running_mean tracks the noise-driven random walk of the bias in front of the BatchNorm: not comparable)
            close(out["state"][k], v, rtol=2e-3, atol=1e-5, what=k)


@pytest.mark.parametrize("name", ["supervised_vae", "triplet"])
def test_trial_loop_restatement_matches_reference_golden_vae_and_triplet(name):
    """The same pin for the other two model classes of the hot path: the VAE's epoch means of mmd_loss and its validation
    total (supervised_vae.py:338-381; z is sampled in eval mode too, so the validation draws are part of the golden) and
    the triplet network's epoch means of triplet_loss over batches of valid anchors with the positives / negatives the
    reference's TripletMultiOmicDataset drew (triplet_encoder.py:276-381, data.py:1102-1131), plus the final
    trainer.validate with its own fresh draws."""
    from oracle import loop
    G = loop_golden_inputs(name)
    out = loop.fit_reference(G["spec"], G["st0"], G["dat"], G["ann"], G["train_idx"], G["val_idx"], batch_size=G["B"],
                             epochs=G["epochs"], lr=G["lr"], patience=0, perms=G["perms"], draws_fn=G["draws"],
                             val_draws_fn=G["val_draws"], batch_fn=G["batch_fn"], val_batch_fn=G["val_batch_fn"])
    exp = loop_golden_expected(G)
    assert len(out["history"]) == G["epochs"] == len(exp)
    want_names = {"supervised_vae": {"mmd_loss", "y", "c", "train_loss", "val_loss"},
                  "triplet": {"triplet_loss", "c", "y", "train_loss", "val_loss"}}[name]
    for e, (got, want) in enumerate(zip(out["history"], exp)):
        assert set(got) == set(want) == want_names, (set(got), set(want))
        for k in want:
            # free-running over the whole trial: the validation loss drifts with the noise-floor biases (see the DirectPred test
            # above); it is pinned tightly from the reference's own weights below
            close(got[k], want[k], rtol=2e-3 if k == "val_loss" else 3e-4, atol=2e-6, what=f"{name} epoch {e} {k}")
        # validation pinned tightly from the REFERENCE's weights at the end of this epoch (same draws / triplets)
        v = loop.validate(G["spec"], G["sub"](f"state_epoch/{e}/"), G["dat"], G["ann"], G["val_idx"], G["B"],
                          (lambda bi, e=e: G["val_draws"](e, bi)) if G["val_draws"] else None,
                          (lambda bi, rows, e=e: G["val_batch_fn"](e, bi, rows)) if G["val_batch_fn"] else None)
        close(v, want["val_loss"], rtol=2e-5, what=f"{name} epoch {e} validation from the reference's state")
    # the final trainer.validate (fresh draws / triplets) from the reference's final weights
    z, E = G["z"], G["epochs"]
    nv = len([k for k in z.keys() if k.startswith(f"val/{E}/") and k.endswith("/n")])
    w = [int(z[f"val/{E}/{bi}/n"]) for bi in range(nv)]
    final_ref = float(np.sum([float(z[f"val/{E}/{bi}/val_loss"]) * w[bi] for bi in range(nv)]) / np.sum(w))
    v = loop.validate(G["spec"], G["sub"]("state_final/"), G["dat"], G["ann"], G["val_idx"], G["B"],
                      (lambda bi: G["val_draws"](E, bi)) if G["val_draws"] else None,
                      (lambda bi, rows: G["val_batch_fn"](E, bi, rows)) if G["val_batch_fn"] else None)
    close(v, final_ref, rtol=2e-5, what=f"{name} final validation")
    close(out["val_loss"], final_ref, rtol=2e-3, what=f"{name} final validation, free-running")
    if name == "triplet":      # loader length = the valid anchors (main.py:176-181): the split indexes them, not the cohort
        n_valid = int((~torch.isnan(G["ann"]["c"])).sum())
        assert G["valid"].numel() == n_valid < G["ann"]["c"].numel()
        assert G["train_idx"].numel() + G["val_idx"].numel() == n_valid and int(G["val_idx"].numel()) == int(n_valid * 0.2)


def test_trial_loop_early_stopping_semantics():
    """EarlyStopping(monitor=val_loss, mode=min, min_delta=0) as documented by Lightning [parity unpinned: Lightning absent]:
    with the golden's own validation curve, patience p stops in the first epoch whose val_loss has not improved on the
    best for p consecutive epochs; objective() then records that 0-based epoch (main.py:319-322)."""
    from oracle import loop
    G = loop_golden_inputs()
    free = loop.fit_reference(G["spec"], G["st0"], G["dat"], G["ann"], G["train_idx"], G["val_idx"], batch_size=G["B"],
                              epochs=G["epochs"], lr=G["lr"], patience=0, perms=G["perms"], draws_fn=G["draws"])
    curve = [r["val_loss"] for r in free["history"]]
    assert any(b >= a for a, b in zip(curve, curve[1:])), "the golden's validation curve must not be monotone"
    for patience in (1, 2, 3):
        best, wait, want = float("inf"), 0, 0
        for e, v in enumerate(curve):
            if v < best:
                best, wait = v, 0
            else:
                wait += 1
                if wait >= patience:
                    want = e
                    break
        out = loop.fit_reference(G["spec"], G["st0"], G["dat"], G["ann"], G["train_idx"], G["val_idx"], batch_size=G["B"],
                                 epochs=G["epochs"], lr=G["lr"], patience=patience, perms=G["perms"], draws_fn=G["draws"])
        assert out["stopped_epoch"] == want, (patience, curve, out["stopped_epoch"])
        assert out["epochs"] == (want if want else G["epochs"])
        assert len(out["history"]) == (want + 1 if want else G["epochs"])
        assert [r["val_loss"] for r in out["history"]] == curve[:len(out["history"])]


def test_attribution_restatement_properties():
    """oracle/attribution.py (Captum absent: the rule is restated) -- completeness of IntegratedGradients: with enough
    Gauss-Legendre nodes the attributions of a sample sum to F(x) - F(0); GradientShap with the quadrature's nodes and
    uniform weights is the same computation with other weights."""
    from oracle import attribution as A
    spec = O.Spec("DirectPred", [("a", 30), ("b", 18)], 6, 0.5, 5, [("y", "numerical", 1), ("c", "categorical", 3)])
    st = {k: v.double() if v.is_floating_point() else v for k, v in O.init_state(spec, seed=4).items()}
    g = torch.Generator().manual_seed(0)
    for k in st:                                   # non-trivial running statistics
        if k.endswith("running_mean"):
            st[k] = torch.randn(st[k].shape, generator=g).double() * 0.3
        if k.endswith("running_var"):
            st[k] = torch.rand(st[k].shape, generator=g).double() + 0.5
    xs = [torch.randn(5, 30, generator=g).double(), torch.randn(5, 18, generator=g).double()]
    al, wt = A.quadrature(64)
    assert abs(sum(wt) - 1.0) < 1e-12 and all(0 < a < 1 for a in al)
    for var, c in (("y", 0), ("c", 2)):
        f1 = A.head_output(spec, st, xs, var)[:, c]
        f0 = A.head_output(spec, st, [torch.zeros_like(x) for x in xs], var)[:, c]
        tot = torch.zeros(5, dtype=torch.float64)
        for a, w in zip(al, wt):
            pts = [(x * a).requires_grad_(True) for x in xs]
            o = A.head_output(spec, st, pts, var)[:, c].sum()
            gr = torch.autograd.grad(o, pts)
            tot += w * sum((g_ * x).sum(1) for g_, x in zip(gr, xs))
        close(tot, f1 - f0, rtol=2e-2, atol=1.5e-3, what=f"IG completeness {var}")     # piecewise-linear net: the ReLU kinks limit the quadrature
    dat = {"a": xs[0], "b": xs[1]}
    imp = A.feature_importance(spec, st, dat, "c", "categorical", 3, "IntegratedGradients", 5, batch_size=2)
    assert set(imp) == {0, 1, 2} and imp[0][0].shape == (30,) and imp[0][1].shape == (18,)
    assert all(float(v.min()) >= 0 for c in imp for v in imp[c])
    al5, _ = A.quadrature(5)
    gs = A.feature_importance(spec, st, dat, "c", "categorical", 3, "GradientShap", 5, batch_size=5, alphas=al5)
    assert gs[1][0].shape == (30,) and not torch.allclose(gs[1][0], imp[1][0])        # same nodes, uniform weights
