"""`sykepic train`: the training workflow on MI355X.

Host-side mirror of the reference's ``sykepic/train/train.py`` (``main`` :17,
``train_net`` :201, ``test_net`` :323): same ``train.ini`` keys, same model
directory artefacts (``config.ini``, ``class_names.txt``,
``class_distribution.csv``, ``best_state.pth``, ``test_report*.txt``), same
``[STAT]``/``[INFO]`` lines, same checkpoint-on-val-accuracy and
early-stop-on-val-loss rules (quirk Q4), same swallowed exceptions (Q5).
The five-line hot loop (zero_grad/forward/loss/backward/step, :239-243)
becomes ``net.forward_backward(x, y)`` + ``optimizer.step()``: fused kernels
in libsykepic_hip.so; loss and accuracy accumulate on the GPU and are read
once per epoch instead of twice per step.

Data parallelism: launched under ``torch.distributed.run`` (one process per
GPU) every rank trains on its shard, gradients are all-reduced over RCCL and
rank 0 alone prints, checkpoints and writes reports.
"""

import contextlib
import os
import shutil
from configparser import ConfigParser
from pathlib import Path

import torch

from . import arch, data, schedule
from . import distill as distill_mod
from . import ema as ema_mod
from . import loss as loss_mod
from . import tta as tta_mod
from .config import (Settings, get_batch_mix, get_distill_info, get_distiller, get_model_ema, get_network,
                     get_transforms)
from . import dp
from .dp import GradSync
from .optim import HipOptimizer


def _dist():
    return dp.init_from_env()


def _check_split(split):
    """`[dataset] split` = fractions for train, validation and (optionally) test; the reference's two complaints."""
    if sum(split) != 1.0:
        raise ValueError(f"Dataset split does not add up to 1.0. Got {sum(split)}")
    if len(split) < 2:
        raise ValueError("Dataset split needs to cover at least train and validation")
    return len(split) == 3


def _png_path(name):
    out = Path(name)
    return out if out.suffix else out.with_suffix(".png")


def main(args):
    config = ConfigParser()
    config.read(args.config)
    cfg = Settings(config)          # config.KEYS: every key of train.ini, parsed on first use
    if not os.environ.get("SYKEPIC_HOST_TRANSFORMS"):
        # the helper process the PNG decode workers are forked from: up before RCCL / HIP exist in this process
        from . import gpu_augment
        gpu_augment.start_decode_server()
    dist, rank, world, local = _dist()
    chief = rank == 0

    ds, im, mo, tr = cfg.dataset, cfg.image, cfg.model, cfg.train
    split, seed = ds.split, ds.random_seed
    test_split = _check_split(split)
    model_data = data.ModelData(ds.path, split, ds.min_N, ds.max_N, ds.exclude, seed)

    # side outputs of the CLI that end the run before any training (`--save-images` only copies)
    if getattr(args, "save_images", None):
        parts = {"train": model_data.train_x, "val": model_data.val_x, "test": model_data.test_x if test_split else []}
        for name, paths in parts.items():
            if paths:
                (Path(args.save_images) / name).mkdir(exist_ok=True, parents=True)
                for p in paths:
                    shutil.copy(p, Path(args.save_images) / name / p.name)
    if getattr(args, "dist", None):
        from . import plots
        plots.dataset_distribution(model_data, _png_path(args.dist))
        print(f"[INFO] Distribution plot saved to {_png_path(args.dist)}")
        return

    if (until := ds.oversample_until) is not None:
        model_data.oversample(until, None)
    elif (decay := ds.oversample_with_decay) is not None:
        model_data.oversample(None, decay)

    img_shape = im.shape
    # test-time augmentation of the test reports (tta.py): a bad mode or a shape it cannot view ends the run here, not
    # behind the last epoch
    test_tta = tr.test_tta
    tta_mod.check_shape(tta_mod.views_of(test_tta), img_shape)
    train_transform, eval_transform = get_transforms(config, img_shape)
    if getattr(args, "collage", None):
        from . import plots
        rows, cols = int(args.collage[0]), int(args.collage[1])
        model_data.set_data_loaders(rows * cols, im.num_workers, train_transform, eval_transform, img_shape[0])
        plots.view_batch(model_data.train_loader, rows, cols, _png_path(args.collage[2]))
        print(f"[INFO] Image collage saved to {_png_path(args.collage[2])}")
        return
    # transforms run batched on the GPU where the pipeline allows it (SYKEPIC_HOST_TRANSFORMS=1: host workers)
    gpu_tf = None if os.environ.get("SYKEPIC_HOST_TRANSFORMS") else torch.device("cuda", local)
    model_data.set_data_loaders(im.batch_size, im.num_workers, train_transform, eval_transform, img_shape[0],
                                rank=rank, world=world, device=gpu_tf)
    num_classes = len(model_data.le.classes_)
    classes = [str(c) for c in model_data.le.classes_]
    # the loss (loss.py): `balanced` weighs by the labels the train loader iterates, oversampled copies included
    train_labels = list(model_data.train_y) + (list(model_data.over_y) if model_data.oversampled else [])
    loss_fn = loss_mod.CrossEntropyLoss(loss_mod.resolve_class_weights(tr.class_weights, classes, train_labels),
                                        tr.label_smoothing)
    checkpoint_on = tr.checkpoint_on
    # Mixup / CutMix (mix.py): None unless `mixup_alpha` or `cutmix_alpha` is set; its own generator, seeded per rank by
    # the rule of the Dropout seed below
    batch_mix = get_batch_mix(config, seed=seed * world + rank)
    # moving average of the weights (ema.py): its settings now, for the resume check; the object once the network exists
    ema_info = ema_mod.describe(tr.ema_decay, tr.ema_warmup)
    external_test = ds.external_test
    if external_test:
        extra_loader = data.extra_eval_dataloader(external_test, model_data, exclude=["Unclassified"])
    # knowledge distillation (distill.py): None unless `distill_from` names a model directory.  Its settings now, for the
    # resume check - a teacher with other classes or another image shape ends the run here; the teacher itself once the
    # network exists
    distill_info = get_distill_info(config, classes, img_shape)

    # `--resume MODEL_DIR`: that directory as it is (no `auto` id, no `exist_ok` complaint, its config.ini / class_names.txt /
    # class_distribution.csv stay), everything else rebuilt from CONFIG as for a fresh run
    resume = getattr(args, "resume", None)
    state = None
    if resume:
        model_dir = Path(resume)
        state = load_train_state(model_dir)
        check_train_state(state, network=mo.network, classes=classes, img_shape=img_shape, optimizer=tr.optimizer,
                          world=world, loss=loss_fn.describe(), checkpoint_on=checkpoint_on,
                          mix=batch_mix.describe() if batch_mix is not None else None, ema=ema_info,
                          distill=distill_info)
    else:
        # model directory <path>/<network>[_<id>]; id "auto" = next free number, picked by rank 0 for the whole job
        # (another rank could already see the directory rank 0 has just made)
        model_id = mo.id
        if model_id == "auto":
            model_id = dp.broadcast_object(data.auto_id(mo.network, mo.path) if chief else None, dist)
        model_dir = mo.path / (mo.network + (f"_{model_id}" if model_id else ""))
    if chief and not resume:
        model_dir.mkdir(parents=True, exist_ok=mo.exist_ok)
        from . import prob as _prob
        _prob.drop_act_means(model_dir)   # exist_ok = yes: means of an earlier run do not belong to the weights about to be written
        model_data.save(model_dir)
        shutil.copy(args.config, model_dir / "config.ini")
        if loss_fn.weight is not None:
            loss_mod.write_weight_file(model_dir, classes, loss_fn.weight)
    if dist is not None:
        dist.barrier()

    if not tr.gpu:
        raise RuntimeError("this build trains on the MI355X only; for `gpu = no` use the reference itself")
    device = torch.device("cuda", local)
    # a resumed run loads every tensor from train_state.pth: no random / pretrained initialisation (and no draw from
    # torch's generator for one)
    net = get_network(config, num_classes, device=device, pretrained_ok=state is None)
    # Dropout masks are a function of (seed, step, layer): give every rank its own stream, otherwise the j-th sample of
    # every shard draws the same mask at every step.  A run stays deterministic for a given random_seed and world size.
    net.set_seed(seed * world + rank)
    if state is None:
        dp.broadcast_state(net, dist)   # every replica starts from rank 0's (random / pretrained) tensors
    schedule.freeze(net.base)
    initial = [p for p in net.parameters() if p.requires_grad]
    optimizer = HipOptimizer(net, tr.optimizer, [{"params": initial, "lr": tr.learning_rate},
                                                 {"params": [], "lr": 0.0}, {"params": [], "lr": 0.0}])
    if chief:
        print("---- Network Head ----")
        print(net.head)

    lr_warmup = lr_scheduler = None
    if (wu := cfg.lr_warmup).use:
        lr_warmup = schedule.LRWarmup(net, optimizer, wu.factor_1, wu.factor_2, wu.step_1, wu.step_2, wu.step_3,
                                      wu.verbose and chief)
    if (red := cfg.lr_reduction).use:
        # quirk Q3: the reference passes `verbose` positionally into `threshold`
        lr_scheduler = schedule.ReduceLROnPlateau(optimizer, "min", red.factor, red.patience, red.verbose)

    run_info = {"network": mo.network, "classes": classes, "img_shape": [int(v) for v in img_shape],
                "optimizer": tr.optimizer, "world": world, "loss": loss_fn.describe(), "checkpoint_on": checkpoint_on}
    if batch_mix is not None:        # (no key without mixing: the file of a run that never heard of it)
        run_info["mix"] = batch_mix.describe()
    if ema_info is not None:         # (likewise)
        run_info["ema"] = ema_info
    if distill_info is not None:     # (likewise)
        run_info["distill"] = distill_info
    if state is not None and (state["early_stopped"] or state["epoch"] >= tr.max_epochs):
        # nothing left to train (raise `max_epochs` to extend a run that reached it): the reports of the best model
        if chief:
            print(f"[INFO] {model_dir}: training ended after epoch {state['epoch']}, nothing to resume")
        best_state = Path(model_dir) / "best_state.pth"
    else:
        # the average starts as a copy of the tensors every replica holds now (a resumed run loads its own over it)
        model_ema = get_model_ema(config, net)
        # every rank loads its own teacher: a second library handle on its device
        distiller = get_distiller(config, classes, img_shape, device)
        best_state = train_net(net, model_data.train_loader, model_data.val_loader, optimizer, loss_fn, tr.max_epochs,
                               tr.early_stop_patience, model_dir, device, lr_scheduler, lr_warmup, dist=dist,
                               run_info=run_info if tr.save_train_state else None, resume=state,
                               checkpoint_on=checkpoint_on, batch_mix=batch_mix, model_ema=model_ema,
                               distiller=distiller)
    if dist is not None:
        dist.barrier()
    net.load_state_dict(torch.load(best_state, map_location="cpu"))
    if chief:
        # activation means of the best model on (this rank's share of) the validation images, stored beside
        # best_state.pth: `sykepic prob` then runs the calibrated single-pass mode (prob.use_act_means)
        from . import prob
        try:
            if not arch.calibrated_mode_ok(net.graph):   # (MobileNetV3: `prob` runs the default mode, nothing to store)
                raise RuntimeError(f"{mo.network} has no calibrated single-pass mode")
            n_cal = prob.calibrate_model(net, model_data.val_loader, 2048)
            if n_cal:
                prob.save_act_means(net, model_dir, n_cal)
                print(f"[INFO] Activation means of {n_cal} validation images saved to {prob.ACT_MEANS_FILE}")
        except Exception as e:  # noqa: BLE001 - an optimisation of later inference, never a reason to lose the run
            prob.drop_act_means(model_dir)     # whatever is there now belongs to other weights
            print(f"[INFO] No activation means stored ({e})")
    tests = ([(None, model_data.test_loader)] if test_split else []) + \
            ([(Path(external_test).name, extra_loader)] if external_test else [])
    for name, loader in tests if chief else []:
        report = test_net(net, loader, model_data.le.classes_, device, test_name=name)
        print(report)
        (model_dir / (f"test_report_{name}.txt" if name else "test_report.txt")).write_text(report)
        if test_tta != "none":
            # the same images again, every one classified in the mode's views: the two accuracies side by side
            report = test_net(net, loader, model_data.le.classes_, device, test_name=name, tta=test_tta)
            print(report)
            (model_dir / (f"test_report_{name}_tta.txt" if name else "test_report_tta.txt")).write_text(report)


TRAIN_STATE_FILE = "train_state.pth"
TRAIN_STATE_FORMAT = 1


def save_atomically(obj, path):
    """`torch.save` into a temporary file of the same directory, then `os.replace`: a kill or an error in the middle of
    the write leaves the previous file as it was."""
    path = Path(path)
    tmp = path.with_name(f"{path.name}.{os.getpid()}.tmp")
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()


def load_train_state(model_dir):
    """`train_state.pth` of a model directory: tensors and plain containers only (`weights_only=True`)."""
    path = Path(model_dir) / TRAIN_STATE_FILE
    if not path.is_file():
        raise FileNotFoundError(f"{path} not found: nothing to resume (the file is written at the end of every epoch "
                                "unless `[train] save_train_state = no`)")
    return torch.load(path, map_location="cpu", weights_only=True)


def _same_mix(a, b):
    """Two `BatchMix.describe()` dicts (None: no mixing) name the same mixing."""
    if not a or not b:
        return not a and not b
    keys = ("mixup_alpha", "cutmix_alpha", "prob", "switch_prob")
    return all(float(a.get(k, -1.0)) == float(b.get(k, -1.0)) for k in keys)


def check_train_state(state, network, classes, img_shape, optimizer, world, loss=None, checkpoint_on="accuracy", mix=None,
                      ema=None, distill=None):
    """A resumed run must be the run that wrote the file: one line naming the first thing that differs.
    loss: `CrossEntropyLoss.describe()` of the config (None: the defaults); a file without the key - every file written
    before the loss had options - was trained with the defaults, and likewise for `checkpoint_on`.
    mix: `BatchMix.describe()` of the config (None: no mixing); a file without the key was written without mixing.
    ema: `ModelEma.describe()` of the config (None: no moving average); a file without the key was written without one.
    distill: `Distiller.describe()` of the config (None: no distillation); a file without the key was written without it."""
    if state.get("format") != TRAIN_STATE_FORMAT:
        raise ValueError(f"cannot resume: train_state.pth has format number {state.get('format')}, this version reads "
                         f"{TRAIN_STATE_FORMAT}")
    for what, key, now in (("network", "network", network), ("class list", "classes", [str(c) for c in classes]),
                           ("image shape", "img_shape", [int(v) for v in img_shape]),
                           ("optimizer", "optimizer", optimizer), ("world size", "world", int(world))):
        was = state[key]
        if was != now:
            if what == "class list":
                diff = sorted(set(was) ^ set(now))
                was, now = f"{len(was)} classes", f"{len(now)} classes (differing: {', '.join(diff[:5]) or 'order'})"
            raise ValueError(f"cannot resume: {what} differs, train_state.pth has {was}, the config gives {now}")
    if not loss_mod.same_loss(state.get("loss"), loss):
        def show(d):
            d = d or {}
            w = d.get("class_weights")
            return (f"label_smoothing {float(d.get('label_smoothing') or 0.0)}, "
                    f"class_weights {'none' if w is None else [round(float(v), 6) for v in w[:4]] + (['...'] if len(w) > 4 else [])}")
        raise ValueError(f"cannot resume: loss differs, train_state.pth has {show(state.get('loss'))}, the config gives "
                         f"{show(loss)}")
    if state.get("checkpoint_on", "accuracy") != checkpoint_on:
        raise ValueError(f"cannot resume: checkpoint_on differs, train_state.pth has {state.get('checkpoint_on', 'accuracy')}, "
                         f"the config gives {checkpoint_on}")
    if not _same_mix(state.get("mix"), mix):
        def show_mix(d):
            return "off" if not d else ", ".join(f"{k} {float(v):g}" for k, v in sorted(d.items()))
        raise ValueError(f"cannot resume: mix differs, train_state.pth has {show_mix(state.get('mix'))}, the config gives "
                         f"{show_mix(mix)}")
    if not ema_mod.same_settings(state.get("ema"), ema):
        raise ValueError(f"cannot resume: ema differs, train_state.pth has {ema_mod.show_settings(state.get('ema'))}, "
                         f"the config gives {ema_mod.show_settings(ema)}")
    if not distill_mod.same_settings(state.get("distill"), distill):
        raise ValueError(f"cannot resume: distill differs, train_state.pth has "
                         f"{distill_mod.show_settings(state.get('distill'))}, the config gives "
                         f"{distill_mod.show_settings(distill)}")


def _rank_state(net, batch_mix=None):
    """What differs from rank to rank: the positions of the generators the shuffle (torch) and the augmentation draws
    (Python's `random`) come from, and the model's mask seed and step counter.  numpy's global generator is not
    saved: nothing on the training path draws from it.  With mixing on, the position of the `BatchMix` generator too
    (`mix_rng`; no such key without it)."""
    import random
    out = {"torch_rng": torch.get_rng_state(), "python_rng": random.getstate(), "model": net.train_counters()}
    if batch_mix is not None:
        out["mix_rng"] = batch_mix.getstate()
    return out


def _sampler_of(loader):
    s = getattr(loader, "sampler", None)
    return s if hasattr(s, "set_epoch") and hasattr(s, "epoch") else None


def collect_train_state(run_info, epoch, ended, early_stopped, net, optimizer, lr_scheduler, book, ranks, train_loader,
                        model_ema=None):
    """Everything `train_net` needs to go on with epoch `epoch + 1` as if it had never stopped.  With a moving average
    the `ema` entry holds its settings, its `tensors` and its count of `updates`; no such key without."""
    sampler = _sampler_of(train_loader)
    out = {
        "format": TRAIN_STATE_FORMAT, **run_info,
        "epoch": int(epoch), "ended": bool(ended), "early_stopped": bool(early_stopped),
        "net": dict(net.state_dict()),
        "optimizer_state": optimizer.state_dict(),     # ("optimizer" is its name, from run_info)
        "groups": [[p.key for p in g["params"]] for g in optimizer.param_groups],
        "requires_grad": {p.key: bool(p.requires_grad) for p in net.parameters()},
        "lr_scheduler": lr_scheduler.state_dict() if lr_scheduler is not None else None,
        "sampler_epoch": int(sampler.epoch) if sampler is not None else None,
        "book": book, "ranks": ranks,
    }
    if model_ema is not None:
        out["ema"] = {**model_ema.describe(), **model_ema.state_dict()}
    return out


def restore_train_state(state, net, optimizer, lr_scheduler, rank, train_loader, batch_mix=None, model_ema=None):
    """Inverse of `collect_train_state`; returns the book-keeping of the epoch loop."""
    import random
    net.load_state_dict(state["net"])       # (the model alone: the average is loaded next)
    if model_ema is not None:
        model_ema.load_state_dict(state["ema"])
    params = dict(net.named_parameters())
    for key, flag in state["requires_grad"].items():
        params[key].requires_grad = flag
    for g, keys in zip(optimizer.param_groups, state["groups"]):   # LRWarmup's edits, by key
        g["params"] = [params[k] for k in keys]
    optimizer.sync_groups()
    optimizer.load_state_dict(state["optimizer_state"])
    if lr_scheduler is not None and state["lr_scheduler"] is not None:
        lr_scheduler.load_state_dict(state["lr_scheduler"])
    sampler = _sampler_of(train_loader)
    if sampler is not None and state["sampler_epoch"] is not None:
        sampler.set_epoch(state["sampler_epoch"])
    mine = state["ranks"][rank]
    net.set_train_counters(mine["model"])
    torch.set_rng_state(mine["torch_rng"])
    random.setstate(mine["python_rng"])
    if batch_mix is not None and "mix_rng" in mine:
        batch_mix.setstate(mine["mix_rng"])
    return state["book"]


def train_net(net, train_dataloader, val_dataloader, optimizer, loss_fn, max_epochs, early_stop_patience,
              model_dir, device, lr_scheduler=None, lr_warmup=None, dist=None, run_info=None, resume=None,
              checkpoint_on="accuracy", batch_mix=None, model_ema=None, distiller=None):
    """loss_fn: None (nn.CrossEntropyLoss() as the reference constructs it), a `loss.CrossEntropyLoss` or a
    `torch.nn.CrossEntropyLoss`: its `weight` and `label_smoothing` go to the loss kernel fused into the training and
    validation steps (`HipNet.set_loss`); another reduction than "mean" is a ValueError.
    checkpoint_on: "accuracy" (the reference's rule) or "balanced_accuracy" - the mean per-class recall of the
    validation pass, from the per-class counters the weighted / smoothed kernel keeps.  With the default loss that
    choice runs the same kernel with unit weights (the same loss up to float32 round-off) for its counters.  With
    any of the three away from its default the validation line also prints `Val Balanced Acc`; with all of them at
    their defaults the step, the lines and the files are those of the plain loss.
    Data parallelism: every rank normalises its loss by the weights of ITS batch (W = sum_i w[y_i]) and the gradients
    are averaged over the ranks, as DistributedDataParallel does - not the mean of one global batch.
    run_info (network, classes, img_shape, optimizer, world): write `train_state.pth` at the end of every epoch;
    resume: the loaded file of an earlier run to continue behind its last finished epoch.
    batch_mix: a `mix.BatchMix` (or None): called once per TRAINING batch, on the device batch, and the step then runs
    the two-label criterion lam * CE(out, y) + (1 - lam) * CE(out, y.roll(1)); the `[STAT] Train Acc` line counts
    against the dominant label of each batch.  Validation and test batches are never mixed.
    model_ema: an `ema.ModelEma` over `net` (or None): updated after every `optimizer.step()`; at the end of an epoch the
    average is swapped in for the validation pass and the `best_state.pth` save, so the `[STAT] Val` lines, the
    checkpoint rule, early stopping and the plateau scheduler see the averaged model, while the `[STAT] Train` lines stay
    those of the raw training forward.  Every rank keeps its own average: the parameters are equal on all ranks by
    construction, the averaged running statistics are averaged over the ranks in front of the validation pass, as the
    raw ones are.  `train_state.pth` is written after swapping back and carries both.
    distiller: a `distill.Distiller` (or None): its teacher classifies every TRAINING batch as the step gets it (behind
    `batch_mix`), and the step's loss is (1 - alpha) * hard + alpha * T^2 * KL(teacher || student); the `[STAT] Train`
    line reports that loss, and a `[STAT] Distill` line behind it the KL term alone and the share of rows whose arg-max
    is the teacher's.  Validation and test run the hard loss alone, so `Val Loss` stays comparable between runs."""
    loss = loss_mod.from_loss_fn(loss_fn)
    if checkpoint_on not in ("accuracy", "balanced_accuracy"):
        raise ValueError(f"checkpoint_on must be accuracy or balanced_accuracy. Got: {checkpoint_on}")
    net = net.to(device)
    chief = dist is None or dist.get_rank() == 0
    parallel = dist is not None and dist.is_initialized() and dist.get_world_size() > 1
    sync = GradSync(net, dist)
    extended = not loss.is_default or checkpoint_on != "accuracy"
    if extended:
        unit = [1.0] * net.num_classes if loss.is_default else None     # (for the counters: see the docstring)
        net.set_loss(loss.weight if unit is None else unit, loss.label_smoothing)
    elif hasattr(net, "set_loss"):
        net.set_loss(None, 0.0)
    max_val_acc, min_val_loss, no_improvement = 0, 0, 0
    train_accs, train_losses, val_accs, val_losses = [], [], [], []
    best_state = Path(model_dir) / "best_state.pth"
    first_epoch = 1
    if resume is not None:
        book = restore_train_state(resume, net, optimizer, lr_scheduler, dp.rank_world(dist)[0], train_dataloader,
                                   batch_mix, model_ema)
        max_val_acc, min_val_loss, no_improvement = book["max_val_acc"], book["min_val_loss"], book["no_improvement"]
        train_accs, train_losses = list(book["train_accs"]), list(book["train_losses"])
        val_accs, val_losses = list(book["val_accs"]), list(book["val_losses"])
        first_epoch = resume["epoch"] + 1
        if chief:
            print(f"[INFO] Resuming after epoch {resume['epoch']}")
    if model_ema is not None and chief:
        print(f"[INFO] Validation, the checkpoint rule and best_state.pth use the moving average of the weights "
              f"({ema_mod.show_settings(model_ema.describe())}); the Train figures are those of the raw weights")
    try:
        from tqdm import tqdm
    except ImportError:  # pragma: no cover
        def tqdm(x, **kw):
            return x
    try:
        for epoch in range(first_epoch, max_epochs + 1):
            if chief:
                print(f"\n----- Epoch {epoch} -----")
            if lr_warmup:
                lr_warmup(epoch)
            net.train()
            net.reset_stats()
            seen = 0
            for batch in (tqdm(train_dataloader) if chief else train_dataloader):
                x, y = batch[0], batch[1]
                optimizer.zero_grad()
                if batch_mix is None and distiller is None:
                    net.forward_backward(x, y)
                else:       # on the device batch: a CPU batch of the host loader is transferred first
                    xm, ya, yb, lam = x.to(device, non_blocking=True), torch.as_tensor(y).to(device), None, 1.0
                    if batch_mix is not None:
                        xm, ya, yb, lam = batch_mix(xm, ya)
                    if distiller is None:
                        net.forward_backward(xm, ya, y2=yb, lam=lam)
                    else:   # the teacher sees what the student is about to see
                        net.forward_backward(xm, ya, y2=yb, lam=lam, teacher_logits=distiller.logits(xm),
                                             distill_alpha=distiller.alpha, distill_temperature=distiller.temperature)
                sync.all_reduce(optimizer)
                optimizer.step()
                if model_ema is not None:
                    model_ema.update()
                seen += len(y)
            loss_sum, correct = net.read_stats()          # one device sync per epoch
            if distiller is not None:
                kd_sum, agree = net.read_distill_stats()
                kd_sum, agree, _ = sync.reduce_stats(kd_sum, agree, seen)
            loss_sum, correct, seen = sync.reduce_stats(loss_sum, correct, seen)
            train_acc, train_loss = correct / seen, loss_sum / seen
            train_accs.append(train_acc)
            train_losses.append(train_loss)
            if chief:
                print(f"[STAT] Train Acc: {train_acc:.3f}, Train Loss: {train_loss:.3f}")
                if distiller is not None:
                    print(f"[STAT] Distill Loss: {kd_sum / seen:.3f}, Teacher Agreement: {agree / seen:.3f}")

            # validation: every rank holds the same model (running statistics averaged), evaluates ITS shard of
            # the validation set, and the counters are summed: checkpoint, early-stop and learning-rate decisions
            # below are then identical on every rank by construction
            dp.sync_buffers(net, dist)
            # with a moving average: the average stands in for the model from here to the checkpoint (and its running
            # statistics are averaged over the ranks as the raw ones were, one line up); the raw weights come back after
            with (model_ema.applied() if model_ema is not None else contextlib.nullcontext()):
                if model_ema is not None:
                    dp.sync_buffers(net, dist)
                net.eval()
                net.reset_stats()
                if extended:
                    net.read_class_counts(reset=True)      # drop the training pass's counts
                seen = 0
                for batch in val_dataloader:
                    net.eval_step(batch[0], batch[1])
                    seen += len(batch[1])
                loss_sum, correct = net.read_stats()
                loss_sum, correct, seen = sync.reduce_stats(loss_sum, correct, seen)
                val_acc, val_loss = correct / seen, loss_sum / seen
                val_accs.append(val_acc)
                val_losses.append(val_loss)
                criterion = val_acc
                if extended:
                    counts = sync.reduce_class_counts(net.read_class_counts(reset=True))
                    val_bal = loss_mod.balanced_accuracy(counts.tolist())
                    if checkpoint_on == "balanced_accuracy":
                        criterion = val_bal
                if chief:
                    if extended:
                        print(f"[STAT] Val Acc: {val_acc:.3f}, Val Loss: {val_loss:.3f}, Val Balanced Acc: {val_bal:.3f}")
                    else:
                        print(f"[STAT] Val Acc: {val_acc:.3f}, Val Loss: {val_loss:.3f}")
                    _plot(train_accs, train_losses, val_accs, val_losses, Path(model_dir), epoch)
                if criterion > max_val_acc:
                    max_val_acc = criterion
                    if chief:
                        print("[INFO] Increased balanced accuracy, saving model state"
                              if checkpoint_on == "balanced_accuracy" else "[INFO] Increased accuracy, saving model state")
                        try:
                            save_atomically(net.state_dict(), best_state)
                        except Exception as e:  # noqa: BLE001 - the previous best model is still there, the run goes on
                            print(f"[INFO] Could not write {best_state.name} ({e}); the previous one stays")
            if val_loss < min_val_loss or epoch == 1:
                no_improvement = 0
                min_val_loss = val_loss
            else:
                no_improvement += 1
                if chief:
                    print(f"[INFO] No reduction in loss for {no_improvement} epochs")
            stop = no_improvement >= early_stop_patience
            if stop:
                if chief:
                    print("[INFO] Stopping early")
            elif lr_scheduler and (not lr_warmup or epoch > lr_warmup.step_3):
                lr_scheduler.step(val_loss)
            if run_info is not None:
                # after every decision of this epoch; the generators stand where the loaders left them (their batch
                # thread has ended with the epoch's last batch), the ranks' positions are gathered into the one file
                ranks = dp.gather_object(_rank_state(net, batch_mix), dist)
                if chief:
                    book = {"max_val_acc": max_val_acc, "min_val_loss": min_val_loss, "no_improvement": no_improvement,
                            "train_accs": train_accs, "train_losses": train_losses, "val_accs": val_accs,
                            "val_losses": val_losses}
                    try:
                        save_atomically(collect_train_state(run_info, epoch, stop or epoch == max_epochs, stop, net,
                                                            optimizer, lr_scheduler, book, ranks, train_dataloader,
                                                            model_ema),
                                        Path(model_dir) / TRAIN_STATE_FILE)
                    except Exception as e:  # noqa: BLE001 - a recovery file, never a reason to lose the run
                        print(f"[INFO] Could not write {TRAIN_STATE_FILE} ({e}); the previous one stays")
            if stop:
                break
    except KeyboardInterrupt:
        print("[INFO] Stopping early")
        sync.close()
    except Exception as e:  # the reference swallows every error here (quirk Q5)
        print(f"[ERROR] {e}")
        if parallel:
            # ... but one replica leaving the loop would leave the others blocked in the next all-reduce:
            # under data parallelism the error ends the rank (non-zero exit; the launcher stops the job)
            raise
    sync.close()
    return best_state


def _plot(train_accs, train_losses, val_accs, val_losses, model_dir, epoch):
    try:
        from . import plots
        plots.plot_stats(train_accs, train_losses, val_accs, val_losses, outfile=model_dir / "train_stats.png",
                         first_epoch=1, epoch_step=3)
        if epoch >= 11:
            plots.plot_stats(train_accs[10:], train_losses[10:], val_accs[10:], val_losses[10:],
                             outfile=model_dir / "train_stats_zoomed.png", first_epoch=11, epoch_step=2)
    except Exception:  # plotting is cosmetic (out of scope)
        pass


def test_net(net, dataloader, classes, device, test_name=None, tta="none"):
    """tta: a mode of tta.MODES; other than `none` the predictions are the arg-max of the probabilities averaged over
    the mode's views (`HipNet.probabilities_tta`), and the first printed line names the mode."""
    net = net.to(device)
    net.eval()
    views = tta_mod.views_of(tta)
    title = "Model Evaluation" + (f" ({test_name})" if test_name else "")
    if tta != "none":
        title += f", test-time augmentation {tta}: {len(views)} views"
    print(f"\n----- {title} -----")
    true_labels, predicted = [], []
    pending = []
    for batch in dataloader:
        x, y = batch[0], batch[1]
        pending.append(((net(x) if tta == "none" else net.probabilities_tta(x, views)).argmax(1), y))
    for preds, y in pending:
        predicted.extend(preds.tolist())
        true_labels.extend(torch.as_tensor(y).tolist())
    acc = sum(int(a == b) for a, b in zip(true_labels, predicted)) / max(1, len(true_labels))
    print(f"[STAT] Test Accuracy: {acc:.3f}\n")
    from sklearn.metrics import classification_report
    return classification_report(true_labels, predicted, target_names=list(classes), zero_division=0)
