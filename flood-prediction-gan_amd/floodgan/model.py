"""Training orchestration for the PairedAttention path, mirroring the reference's
`Model` (models/model.py:26-160) and `Model.train_paired` (models/model.py:598-658).

`PairedStep` is the fused device iteration: the exact sequence of models/model.py:615-646
(G forward; D step on fake(detached)+real with LSGAN MSE x0.5 and Adam(D); G step on the
UPDATED D with MSE(D(fake),1) + 100*L1 and Adam(G)) executed by the native executors with
no autograd graph, one fused 2N-image discriminator pass for the D step (InstanceNorm is
per-sample, so D(fake) and D(real) in one batch is the same computation), fused losses and
FusedAdam.  With torch.distributed initialised it performs batch-DP over RCCL.
"""
import itertools
import time

import numpy as np
import torch
from torch import nn
from torch.optim import lr_scheduler

from . import executor as X
from . import ops
from . import pix2pix as P2P
from .cycle import IDENTITY_KEYS, LOSS_KEYS, CycleStep
from .model_architectures import (AttentionGANDiscriminator, AttentionGANGenerator, CycleGANDiscriminator,
                                  CycleGANGenerator, PairedAttentionDiscriminator, PairedAttentionGenerator,
                                  Pix2PixDiscriminator, Pix2PixGenerator)
from .optim import FusedAdam
from .parallel import FlatGrads, world

TOPOGRAPHY_CHANNELS = {"all": 9, "map": 6, "dem": 4, "flow": 4, "river": 4, None: 3}


class PairedStep:
    """One paired-GAN training iteration on device tensors x [N,C,H,W], y [N,3,H,W].
    Returns a device tensor [D real, D synthetic, G synthetic, 100*L1] (models/model.py:648-651).

    fake_loss (None by default): an extra generator term, an object with a `weight` and a call
    fake_loss(fake, y, g_fake, scale) made between the L1 term and the G step's discriminator backward; it adds
    scale * dL/d(fake) into g_fake (scale = weight / world size) and returns weight * L as a one-element device
    tensor, which becomes a fifth entry of the returned losses (FloodMaskLoss.fused_term is one)."""

    fake_loss = None

    def __init__(self, generator, discriminator, opt_g, opt_d, group=None):
        self.G, self.D = generator, discriminator
        self.opt_g, self.opt_d = opt_g, opt_d
        self.gp, self.dp = generator.param_dict(), discriminator.param_dict()
        # gradient buffers laid out in the order the backward completes them: each bucket's RCCL
        # all-reduce starts as soon as it is written and overlaps the rest of the backward
        self.gflat = FlatGrads(self.gp, self._net.gen_bucket_names())
        self.dflat = FlatGrads(self.dp, self._net.disc_bucket_names())
        self.group = group
        self.last_mask = None
        self.last_output = None
        # test instrumentation: when True, each call stores the activation decisions of its three
        # networks' passes in self.decisions ({"G": [...], "D": [fake, real, G-step]}, oracle order) and the
        # L1 term's sign decisions ({"L1": [{"l1": sign(fake - y)}]})
        self.record_decisions = False
        self.decisions = None
        # test instrumentation (teacher forcing): discriminator parameters {name: tensor} that replace the
        # result of Adam(D) before the G step, so that another implementation's G half can be compared on
        # the same discriminator (the oracle's d_after); the step's own Adam(D) result is kept in d_after_own
        self.d_after = None
        self.d_after_own = None

    # ---- the networks: what a subclass running the same iteration on other executors overrides.  _net is the
    # executor module, for what both spell alike (bucket orders, gen_backward, disc_backward, *_act_decisions);
    # the two forwards take different arguments
    _net = X

    def _gen_forward(self, x):
        """-> (fake, attention mask or None, saved)"""
        return X.gen_forward(self.gp, x, save=True)

    def _disc_forward(self, dinp, groups):
        """groups: the separate discriminator calls of the reference stacked along dinp's batch"""
        return X.disc_forward(self.dp, dinp, save=True)      # InstanceNorm is per sample: one batch is the same

    def __call__(self, x, y):
        ws, _ = world()
        inv = 1.0 / ws
        N, C, H, W = x.shape
        dev = x.device
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        # (the flat gradient views are attached right before each backward: the per-parameter checks then run on
        # the host while the GPU works through the forward instead of ahead of the step's first launch)
        # generator forward                                           (models/model.py:615)
        fake, mask, gS = self._gen_forward(x)
        # ---- discriminator step: fake (detached) and real in one 2N batch   (:620-633)
        dinp = X.disc_pack([(x, fake), (x, y)], C + 3)
        pred, dS = self._disc_forward(dinp, 2)
        g_pred = torch.empty_like(pred)
        ops.mse_const(pred[:N], 0.0, 0.5 * inv, losses[1:2], g_pred[:N])
        ops.mse_const(pred[N:], 1.0, 0.5 * inv, losses[0:1], g_pred[N:])
        net = self._net
        rec = None
        if self.record_decisions:
            rec = {"G": [net.gen_act_decisions(gS)],
                   "D": [net.disc_act_decisions(dS, 0, N), net.disc_act_decisions(dS, N)]}
        self.dflat.attach()
        self.dflat.begin(self.group)
        net.disc_backward(self.dp, dS, g_pred, param_grads=True, grads_into=self._grads(self.dp),
                          ready=self.dflat.ready)
        del dS
        self.dflat.finish()
        self.opt_d.step()
        if self.d_after is not None:
            self.d_after_own = {k: p.detach().clone() for k, p in self.D.named_parameters()}
            with torch.no_grad():
                for k, p in self.D.named_parameters():
                    p.copy_(self.d_after[k])
        # ---- generator step against the updated discriminator                 (:636-646)
        dinp = X.disc_prefix(dinp, N)          # (x, fake): the D step's first half, unchanged since
        pred, dS = self._disc_forward(dinp, 1)
        g_pred = torch.empty_like(pred)
        ops.mse_const(pred, 1.0, inv, losses[2:3], g_pred)
        g_fake = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
        ops.l1(fake, y, 100.0 * inv, losses[3:4], g_fake, loss_scale=100.0)     # logged as 100 * L1 (:643-651)
        if self.fake_loss is not None:
            losses = torch.cat([losses, self.fake_loss(fake, y, g_fake, self.fake_loss.weight * inv)])
        net.disc_backward(self.dp, dS, g_pred, param_grads=False, input_grad=g_fake, input_grad_channels=(C, 3),
                          input_grad_accumulate=True)
        if rec is not None:
            rec["D"].append(net.disc_act_decisions(dS))
            rec["L1"] = [{"l1": torch.sign(fake.detach() - y)}]   # the L1 term's sign decisions (-1 / 0 / +1)
            self.decisions = rec
        del dS, dinp
        self.gflat.attach()
        self.gflat.begin(self.group)
        net.gen_backward(self.gp, gS, g_fake, grads_into=self._grads(self.gp), ready=self.gflat.ready)
        del gS
        self.gflat.finish()
        self.opt_g.step()
        self.last_mask, self.last_output = mask, fake
        return losses

    @staticmethod
    def _grads(params):
        return {k: p.grad for k, p in params.items()}


class Pix2PixStep(PairedStep):
    """The same iteration (models/model.py:611-651) for Pix2Pix: BatchNorm in training mode, so the D
    step's D(fake) and D(real) -- separate calls in the reference -- run as one 2N pass with two
    BatchNorm groups (per-half statistics, two running-stat updates in order), and the G step's D call
    updates the discriminator's running statistics a third time.  With dropout_rng "host" the generator's Dropout
    masks are torch's CPU stream in the reference's order, regenerated on the device (floodgan.torch_rng)."""

    _net = P2P

    def __init__(self, generator, discriminator, opt_g, opt_d, group=None):
        super().__init__(generator, discriminator, opt_g, opt_d, group)
        self.gb, self.db = generator.buffer_dict(), discriminator.buffer_dict()
        self.masks = None        # test hook: dropout masks to use instead of drawing
        self.last_masks = None

    def __call__(self, x, y):
        N, C, H, W = x.shape
        commit = None
        if self.masks is not None:
            masks = self.masks
        elif self.G.dropout_rng == "host":
            masks, commit = P2P.draw_dropout_deferred(N, H, W, x.device)
        else:
            masks = P2P.draw_dropout(N, H, W, self.G.dropout_rng, x.device)
        self.last_masks = masks
        try:
            return super().__call__(x, y)
        finally:
            # torch's CPU generator advanced past this iteration's Dropout draws -- also when the iteration raised
            # (its masks were drawn: a retry must not reuse them); commit() raises if anything drew in between
            if commit is not None:
                commit()

    def _gen_forward(self, x):
        fake, gS = P2P.gen_forward(self.gp, self.gb, x, masks=self.last_masks, training=True, save=True)
        return fake, None, gS

    def _disc_forward(self, dinp, groups):
        return P2P.disc_forward(self.dp, self.db, dinp, groups=groups, training=True, save=True)


class Model:
    """The reference's Model (models/model.py:26-160) with identical construction semantics (seed,
    initialise_weights, Adam(2e-4, (0.5, 0.999)), LambdaLR) for "PairedAttention" (train_paired,
    the hot path) and the cycle models "AttentionGAN" / "CycleGAN" (train_cycle)."""

    def __init__(self, model="PairedAttention", dataset_subset="all", dataset_dem="best", data_path=None,
                 num_epochs=1, topography="all", resize=256, crop=None, save_model_interval=0,
                 save_images_interval=0, verbose=False, load_pretrained_model=False, pretrained_model_path=None,
                 add_identity_loss=False, training_model=True, seed=47, device="cuda", train_loader=None,
                 val_loader=None, test_loader=None, batch_size=1, num_workers=0,
                 csv_path="metadata/dataset_split.csv", flood_mask_weight=0.0, segmentation_model_path=None,
                 flood_mask_batch_stats=False):
        # flood_mask_weight > 0 (not a keyword of the reference's): the paired step's generator also descends
        # weight * FloodMaskLoss(fake, target) of the segmentation U-Net at segmentation_model_path
        self.flood_mask_weight = float(flood_mask_weight)
        self.segmentation_model_path, self.flood_mask_batch_stats = segmentation_model_path, flood_mask_batch_stats
        if self.flood_mask_weight < 0:
            raise ValueError(f"flood_mask_weight must be >= 0 (got {flood_mask_weight})")
        if self.flood_mask_weight > 0 and not segmentation_model_path:
            raise ValueError("flood_mask_weight > 0 needs segmentation_model_path: the checkpoint of the trained "
                             "segmentation U-Net the flood-mask loss is measured with")
        saved = None
        if load_pretrained_model:
            # models/model.py:52-57: the checkpoint, not the `model` argument, names the architecture
            saved = torch.load(pretrained_model_path, map_location="cpu", weights_only=True)
            model = saved["model"]
        self.model = model.lower()
        if self.model not in ("pairedattention", "pix2pix", "attentiongan", "cyclegan"):
            raise NotImplementedError("Model must be one of: Pix2Pix, CycleGAN, AttentionGAN or PairedAttention")
        if saved is not None:
            self.num_epochs, self.topography = saved["num_epochs"], saved["topography"]
            self.add_identity_loss = saved["add_identity_loss"]
        else:
            self.num_epochs, self.topography, self.add_identity_loss = num_epochs, topography, add_identity_loss
        self.verbose, self.save_model_interval = verbose, save_model_interval
        self.save_images_interval = save_images_interval
        self.load_pretrained_model, self.data_path = load_pretrained_model, data_path
        self.dataset_subset, self.dataset_dem, self.resize, self.crop = dataset_subset, dataset_dem, resize, crop
        self.training_model, self.seed, self.device = training_model, seed, device
        self.model_is_cycle = self.model in ("attentiongan", "cyclegan")
        self.model_is_attention = self.model in ("pairedattention", "attentiongan")     # models/model.py:219-229
        if self.flood_mask_weight > 0 and self.model_is_cycle:
            raise NotImplementedError("the flood-mask loss is a term of the paired step (PairedAttention, Pix2Pix)")

        input_channels = TOPOGRAPHY_CHANNELS[self.topography]
        torch.manual_seed(self.seed)
        if self.model_is_cycle:                                   # models/model.py:96-100, :108-115
            self._init_cycle(input_channels, device)
        else:
            gcls, dcls = ((Pix2PixGenerator, Pix2PixDiscriminator) if self.model == "pix2pix"
                          else (PairedAttentionGenerator, PairedAttentionDiscriminator))
            self.generator = gcls(input_channels=input_channels).apply(self.initialise_weights).to(device)
        if self.training_model and not self.model_is_cycle:
            self.discriminator = dcls(input_channels=input_channels).apply(self.initialise_weights).to(device)
            self.optimizer_discriminator = FusedAdam(self.discriminator.parameters(), lr=0.0002, betas=(0.5, 0.999))
            self.optimizer_generator = FusedAdam(self.generator.parameters(), lr=0.0002, betas=(0.5, 0.999))
        if self.training_model:
            self.scheduler_generator = lr_scheduler.LambdaLR(self.optimizer_generator, lr_lambda=self.lambda_rule)
            self.scheduler_discriminator = lr_scheduler.LambdaLR(self.optimizer_discriminator,
                                                                 lr_lambda=self.lambda_rule)
        if saved is not None and self.model_is_cycle:
            self.starting_epoch, self.all_losses = saved["starting_epoch"], saved["all_losses"]
            for name in self._cycle_nets():
                getattr(self, name).load_state_dict(saved[name])
            if self.training_model:
                for name in ("optimizer_generator", "optimizer_discriminator", "scheduler_generator",
                             "scheduler_discriminator"):
                    getattr(self, name).load_state_dict(saved[name])
        elif saved is not None:
            self.starting_epoch, self.all_losses = saved["starting_epoch"], saved["all_losses"]
            self.generator.load_state_dict(saved["generator"])
            if self.training_model:
                self.discriminator.load_state_dict(saved["discriminator"])
                self.optimizer_discriminator.load_state_dict(saved["optimizer_discriminator"])
                self.optimizer_generator.load_state_dict(saved["optimizer_generator"])
                self.scheduler_discriminator.load_state_dict(saved["scheduler_discriminator"])
                self.scheduler_generator.load_state_dict(saved["scheduler_generator"])
        else:
            self.starting_epoch = 1
            self.all_losses = self.initialise_loss_storage(overall=True)
        self.current_epoch = self.starting_epoch
        # the data (models/model.py:150-156): with a data_path the three loaders are built as the reference
        # builds them -- floodgan.data's staged TileLoaders over the same split table (csv_path: the
        # reference reads metadata/dataset_split.csv relative to the working directory), batch_size images
        # per step (the reference's is 1) and, under torch.distributed, this rank's shard of every global
        # batch.  Loaders passed in explicitly (any iterable of (input, target, names)) take precedence.
        self.batch_size = batch_size
        if data_path is not None and train_loader is None:
            from .data import create_flood_dataset
            ws, rank = world()
            train_loader, val_loader, test_loader = create_flood_dataset(
                dataset_subset, dataset_dem, data_path, self.topography, resize=resize, crop=crop,
                batch_size=batch_size, num_workers=num_workers, csv_path=csv_path, device=device, rank=rank, world=ws)
        self.train_loader, self.val_loader, self.test_loader = train_loader, val_loader, test_loader
        self.csv_path = csv_path
        self._step = None

    def _cycle_nets(self):
        nets = ["pre_to_post_generator", "post_to_pre_generator"]
        return nets + (["pre_discriminator", "post_discriminator"] if self.training_model else [])

    def _init_cycle(self, input_channels, device):
        """models/model.py:96-100 (construction order = RNG order) and :108-115 (optimisers)."""
        gcls, dcls = ((AttentionGANGenerator, AttentionGANDiscriminator) if self.model == "attentiongan"
                      else (CycleGANGenerator, CycleGANDiscriminator))
        for name in self._cycle_nets():
            cls = gcls if name.endswith("generator") else dcls
            setattr(self, name, cls(input_channels=input_channels).apply(self.initialise_weights).to(device))
        if self.training_model:
            self.optimizer_generator = FusedAdam(itertools.chain(self.pre_to_post_generator.parameters(),
                                                                 self.post_to_pre_generator.parameters()),
                                                 lr=0.0002, betas=(0.5, 0.999))
            self.optimizer_discriminator = FusedAdam(itertools.chain(self.post_discriminator.parameters(),
                                                                     self.pre_discriminator.parameters()),
                                                     lr=0.0002, betas=(0.5, 0.999))

    @staticmethod
    def initialise_weights(m):
        """models/model.py:162-173"""
        classname = m.__class__.__name__
        if hasattr(m, "weight") and (classname.find("Conv") != -1 or classname.find("Linear") != -1):
            nn.init.normal_(m.weight.data, 0.0, 0.02)
            if hasattr(m, "bias") and m.bias is not None:
                nn.init.constant_(m.bias.data, 0.0)
        elif classname.find("BatchNorm2d") != -1:
            nn.init.normal_(m.weight.data, 1.0, 0.02)
            nn.init.constant_(m.bias.data, 0.0)

    def lambda_rule(self, epoch):
        """models/model.py:175-181"""
        return 1.0 - max(0, epoch + 1 - (self.num_epochs / 2)) / float((self.num_epochs / 2) + 1)

    def initialise_loss_storage(self, overall):
        """models/model.py:183-205"""
        pre = "all_" if overall else ""
        if self.model_is_cycle:
            keys = LOSS_KEYS + (IDENTITY_KEYS if self.add_identity_loss else [])
            return {pre + k: [] for k in keys}
        return {pre + k: [] for k in self.paired_loss_keys()}

    def paired_loss_keys(self):
        """the reference's four keys, in the order the fused step returns its losses; the flood-mask term's when on"""
        keys = ["losses_discriminator_real", "losses_discriminator_synthetic", "losses_generator_synthetic",
                "l1_losses_generator_synthetic"]
        return keys + (["losses_flood_mask_generator_synthetic"] if self.flood_mask_weight > 0 else [])

    @property
    def step_fn(self):
        if self._step is None:
            cls = Pix2PixStep if self.model == "pix2pix" else PairedStep
            self._step = cls(self.generator, self.discriminator, self.optimizer_generator, self.optimizer_discriminator)
            if self.flood_mask_weight > 0:
                from .segmentation import FloodMaskLoss
                with torch.random.fork_rng(devices=[]):      # (the U-Net is initialised before its checkpoint loads)
                    loss = FloodMaskLoss(self.segmentation_model_path, batch_stats=self.flood_mask_batch_stats)
                self.flood_mask_loss = loss.to(self.device)
                self._step.fake_loss = loss.fused_term(self.flood_mask_weight)
        return self._step

    def train_paired(self):
        """models/model.py:598-658 on the fused device step."""
        if self.train_loader is None:
            raise RuntimeError("no training data: pass data_path (floodgan.data loaders, as models/model.py:150-156) "
                               "or train_loader (an iterable of (input, target, names))")
        keys = self.paired_loss_keys()
        for epoch in range(self.starting_epoch, self.num_epochs + 1):
            t0 = time.time()
            losses = self.initialise_loss_storage(overall=False)
            self.discriminator.train()
            self.generator.train()
            torch.manual_seed(epoch)
            for input_stack, output_image, _ in self.train_loader:
                input_stack = input_stack.to(self.device, non_blocking=True)
                output_image = output_image.to(self.device, non_blocking=True)
                vals = self.step_fn(input_stack, output_image).cpu().tolist()
                for k, v in zip(keys, vals):
                    losses[k].append(v)
            self.scheduler_discriminator.step()
            self.scheduler_generator.step()
            self.save_results(epoch, losses, t0)

    @property
    def cycle_step_fn(self):
        if self._step is None:
            self._step = CycleStep(self.pre_to_post_generator, self.post_to_pre_generator, self.pre_discriminator,
                                   self.post_discriminator, self.optimizer_generator, self.optimizer_discriminator,
                                   identity=self.add_identity_loss)
        return self._step

    def train_cycle(self):
        """models/model.py:660-758 on the fused device step (CycleStep)."""
        if not self.model_is_cycle:
            raise RuntimeError("train_cycle needs model='AttentionGAN' or 'CycleGAN'")
        if self.train_loader is None:
            raise RuntimeError("no training data: pass data_path (floodgan.data loaders, as models/model.py:150-156) "
                               "or train_loader (an iterable of (input, target, names))")
        for epoch in range(self.starting_epoch, self.num_epochs + 1):
            t0 = time.time()
            losses = self.initialise_loss_storage(overall=False)
            for name in self._cycle_nets():
                getattr(self, name).train()
            torch.manual_seed(epoch)
            for input_stack, output_image, _ in self.train_loader:
                input_stack = input_stack.to(self.device, non_blocking=True)
                output_image = output_image.to(self.device, non_blocking=True)
                vals = self.cycle_step_fn(input_stack, output_image).cpu().tolist()
                for k, v in zip(losses.keys(), vals):
                    losses[k].append(v)
            self.scheduler_generator.step()
            self.scheduler_discriminator.step()
            self.save_results(epoch, losses, t0)

    def calculate_metrics(self, use_test_data=False, seg_model_path=None, seg_model=None, lpips_weights=None):
        """models/model.py:363-422 on the device (floodgan.evaluate): the generator (pre_to_post for the
        cycle models) over the validation / test loader, PSNR / SSIM / MS-SSIM of its [0, 1] outputs,
        the segmentation U-Net's flood masks of output and target and their binary metrics; LPIPS when
        lpips_weights (a path, a dict or a floodgan.evaluate.LPIPS object) is given, else NaN.  Returns
        the one-row DataFrame the reference prints (and writes it under data_path/metrics/ when set)."""
        import pandas as pd

        from .evaluate import calculate_metrics, segmentation_model
        loader = self.test_loader if use_test_data else self.val_loader
        if loader is None:
            raise RuntimeError("assign Model.val_loader / Model.test_loader first (floodgan.data.create_flood_dataset)")
        seg = seg_model if seg_model is not None else segmentation_model(seg_model_path, self.device)
        gen = self.pre_to_post_generator if self.model_is_cycle else self.generator
        res = calculate_metrics(gen, loader, seg, self.topography, self.device, lpips_weights=lpips_weights)
        # the reference's table (models/model.py:419-422): one row, a "0" index column, written to
        # create_path("metric")
        df = pd.DataFrame([(k, v) for k, v in res.items()]).set_index(0).transpose()
        if self.verbose:
            print(df)
        if self.data_path:
            import os
            path = self.create_path("metric")
            os.makedirs(os.path.dirname(path), exist_ok=True)
            df.to_csv(path)
        return df

    def prettify_model_name(self, model_name=None):
        """models/model.py:231-239"""
        pretty = {"pix2pix": "Pix2Pix", "cyclegan": "CycleGAN", "attentiongan": "AttentionGAN",
                  "pairedattention": "PairedAttention"}
        return pretty[model_name.lower()] if model_name else pretty[self.model]

    def create_path(self, save_type, info=""):
        """models/model.py:241-258: the reference's file naming for models, metrics and images"""
        from datetime import datetime
        ext = {"image": ".png", "figure": ".png", "model": ".pth.tar", "metric": ".csv"}[save_type]
        now = str(datetime.now())[:-7].replace(" ", "-").replace(":", "-")
        identity = f"identity{self.add_identity_loss}" if self.model_is_cycle else ""
        path = (f"{self.data_path}/{save_type}s/"
                f"{self.prettify_model_name()}_{info}_epoch"
                f"{self.current_epoch if self.training_model else self.current_epoch - 1}_"
                f"{self.topography}Topography_{identity}_"
                f"{self.dataset_subset}Data_{self.dataset_dem}DEM_"
                f"resize{self.resize}_crop{self.crop}_"
                f"date{now}{ext}")
        return path.replace("__", "_")

    def save_results(self, epoch, losses, epoch_start_time):
        """models/model.py:322-361: loss bookkeeping, checkpoint and, every save_images_interval epochs, the sample
        image sheets (plot_sample_images).  The loss-curve figure (plot_losses) is a matplotlib line chart and is
        not drawn here."""
        self.current_epoch = epoch
        for key in self.all_losses.keys():
            self.all_losses[key].append(float(np.mean(losses[key[4:]])))
        if self.verbose:
            print(f"Epoch {epoch} ({time.time() - epoch_start_time:.2f} seconds) | "
                  + " | ".join(f"{k} = {v[-1]:.2f}" for k, v in self.all_losses.items()))
        if self.save_model_interval != 0 and epoch % self.save_model_interval == 0:
            path = self.create_path("model")                      # models/model.py:355-357
            if self.verbose:
                print(f"Saving {self.prettify_model_name()} model to {path}")
            torch.save(self.checkpoint(epoch), path)
        if self.save_images_interval != 0 and epoch % self.save_images_interval == 0:      # models/model.py:360-361
            self.plot_sample_images(num_images=5, use_test_data=False)

    # ---- pictures (models/model.py:475-596) on floodgan.render: converted and composed on the device

    def plot_image(self, image_name, plot_single_image, plot_image_set, crop_index=0):
        """models/model.py:475-540: the tile pair `image_name` through the generator (pre_to_post for the cycle
        models) under torch.manual_seed(47).  plot_single_image: "input", "ground truth", "output" or "attention
        mask" written with the reference's file names and plt.imsave's bytes; plot_image_set: one sheet input |
        output | [attention mask] | ground truth (floodgan.render.save_sheet: panels at native resolution, no
        titles) at create_path("image", info=name).  Returns {"input" | ... | "set": path} of the files written."""
        import os

        from .data import load_image_pair
        from .render import save_image, save_sheet
        x, y, name = load_image_pair(image_name, self.data_path, self.dataset_dem, self.topography, self.resize,
                                     self.crop, crop_index, csv_path=self.csv_path, device=self.device)
        generator = self.pre_to_post_generator if self.model_is_cycle else self.generator
        torch.manual_seed(47)
        with torch.no_grad():
            out = generator(x)
        os.makedirs(f"{self.data_path}/images", exist_ok=True)
        written = {}
        if plot_single_image:
            if plot_single_image == "input":
                written["input"] = save_image(f"{self.data_path}/images/{name}_input.png", x, "rgb")
            elif plot_single_image == "ground truth":
                written["ground truth"] = save_image(f"{self.data_path}/images/{name}_groundTruth.png", y, "rgb")
            elif plot_single_image == "output":
                written["output"] = save_image(self.create_path("image", info=name), out, "rgb")
            elif plot_single_image == "attention mask" and self.model_is_attention:
                written["attention mask"] = save_image(self.create_path("image", info=f"{name}_attentionMask"),
                                                       generator.last_attention_mask, "attention")
            else:
                raise NotImplementedError("Type of image must be one of 'input', 'ground truth', 'output', or "
                                          "'attention mask'")
            if self.verbose:
                print(f"Saving {plot_single_image} of image '{name}' to {written[plot_single_image]}")
        if plot_image_set:
            path = self.create_path("image", info=name)
            self.last_panels = save_sheet(path, self._sheet_columns([x], [out], [generator.last_attention_mask]
                                                                    if self.model_is_attention else None, [y]), [name])
            written["set"] = path
            if self.verbose:
                print(f"Saving {name} image set to {path}")
        return written

    def predict_scene(self, input_path, tile=None, overlap=64, batch=8, seg_model_path=None, batch_stats=False,
                      out_dir=None, min_region=None, min_hole=None, connectivity=8, depth=False, pixel_area=1.0,
                      depth_vmax=None, polygons=False, transform=None, drainage=False, flat_rounds=0):
        """Not in the reference: the predicted post-flood picture of a whole pre-flood scene, a TIFF of any size that
        need not be a dataset tile (floodgan.data.load_scene, floodgan.scene.predict_scene: overlapping windows
        through the generator -- pre_to_post for the cycle models -- blended on the device).  tile=None: the size the
        model was built for (resize when set, else 512).  Writes {out_dir}/{name}_prediction.png (out_dir defaults
        to {data_path}/images) and, with seg_model_path (a checkpoint path, a SegmentationModel or a UNet), the flood
        mask of the blended segmentation logits as {name}_floodMask.png.  Returns {"prediction": path, "flood_mask":
        path or None, "flood_fraction": float or None, "grid": (ys, xs)}.  With min_region / min_hole (either given; they
        need seg_model_path) the mask is sieved (floodgan.regions: flood components below min_region pixels removed,
        enclosed holes below min_hole filled, `connectivity` 8 or 4 for the flood class): {name}_floodMask.png is then
        the sieved mask, {name}_floodRegions.csv beside it lists the regions, and the returned dict gains "regions"
        (the CSV's path) and "region_count".  With depth=True (it needs seg_model_path and a 9-channel file, whose
        channel 3 is the elevation: floodgan.data.load_scene_elevation) the flood depth of the mask
        (floodgan.depth.flood_depth with `pixel_area`) is written as {name}_floodDepth.png -- the "attention"
        rendering of clamp(depth / vmax, 0, 1), vmax = depth_vmax, or the scene's maximum depth, or 1 when that is
        0 --, {name}_floodMask.png and {name}_floodRegions.csv are written as with the minima (off unless given),
        the CSV with the depth columns, and the returned dict gains "flood_depth" (the picture's path), "max_depth",
        "mean_depth" and "volume".  With polygons=True (it needs seg_model_path) the regions are traced into
        polygons on the device (floodgan.outline) and written as {name}_floodRegions.geojson beside the CSV -- one
        Polygon per region with the CSV's columns as properties, positions [x, y] in pixel corners or, with
        `transform` (a GDAL-order 6-tuple), in its coordinates -- with the mask and the CSV as with the minima (off
        unless given); the returned dict gains "polygons" (the file's path).  With drainage=True (a 9-channel file;
        seg_model_path is not needed) the drainage of the elevation (floodgan.flow.flow_accumulation with
        `flat_rounds`) is written as {name}_flowAccumulation.png -- the "attention" rendering of
        floodgan.flow.render_flow --, the CSV and the GeoJSON, where they are written, gain max_accumulation and
        pit_pixels, and the returned dict gains "flow_accumulation" (the picture's path) and "pit_count".  Out of
        scope: attention-mask mosaics,
        reflect-padding of scenes smaller than a window, GeoTIFF output."""
        import os

        from .data import load_scene, load_scene_elevation
        from .render import save_image
        from .scene import predict_scene, scene_name
        if out_dir is None:
            if self.data_path is None:
                raise ValueError("predict_scene: pass out_dir (the default is {data_path}/images and this Model has "
                                 "no data_path)")
            out_dir = f"{self.data_path}/images"
        if tile is None:
            tile = self.resize if self.resize else 512
        elevation = None
        if polygons and seg_model_path is None:
            raise ValueError("predict_scene: polygons=True outlines the regions of the flood mask and needs "
                             "seg_model_path")
        if depth:
            if seg_model_path is None:
                raise ValueError("predict_scene: depth=True gives the depth of the flood mask and needs seg_model_path")
            if depth_vmax is not None and not depth_vmax > 0:
                raise ValueError(f"predict_scene: depth_vmax {depth_vmax!r} must be positive")
            elevation = load_scene_elevation(input_path, self.device)
        if drainage:
            from .flow import check_flat_rounds
            flat_rounds = check_flat_rounds(flat_rounds)
            dem = elevation if elevation is not None else load_scene_elevation(input_path, self.device)
        x = load_scene(input_path, self.topography, self.device)
        generator = self.pre_to_post_generator if self.model_is_cycle else self.generator
        res = predict_scene(generator, x, tile=tile, overlap=overlap, batch=batch, seg_model=seg_model_path,
                            batch_stats=batch_stats, min_region=min_region, min_hole=min_hole,
                            connectivity=connectivity, elevation=elevation, pixel_area=pixel_area,
                            polygons=bool(polygons))
        if drainage:                # (here and not through predict_scene: its elevation would also ask for the depth)
            from .scene import add_drainage
            add_drainage(res, dem, flat_rounds)
        os.makedirs(out_dir, exist_ok=True)
        name = scene_name(input_path)
        written = {"prediction": save_image(f"{out_dir}/{name}_prediction.png", res["output"], "rgb"),
                   "flood_mask": None, "flood_fraction": res.get("flood_fraction"), "grid": res["grid"]}
        if "flood_mask" in res:
            from .regions import write_regions_csv
            written["flood_mask"] = save_image(f"{out_dir}/{name}_floodMask.png", res["flood_mask"], "mask_true")
            written["regions"] = write_regions_csv(f"{out_dir}/{name}_floodRegions.csv", res["regions"],
                                                   res.get("depth"), res.get("flow"))
            written["region_count"] = res["regions"]["count"]
            if polygons:
                from .outline import write_regions_geojson
                written["polygons"] = write_regions_geojson(f"{out_dir}/{name}_floodRegions.geojson", res["regions"],
                                                            res["outlines"], res.get("depth"), transform,
                                                            res.get("flow"))
            if depth:
                vmax = depth_vmax if depth_vmax is not None else (res["depth"]["max_depth"] or 1.0)
                # (a tensor divisor: one correctly rounded fp32 division per pixel, not a product with 1 / vmax)
                unit = torch.clamp(res["flood_depth"] / torch.tensor(float(vmax), dtype=torch.float32,
                                                                      device=res["flood_depth"].device), 0.0, 1.0)
                written["flood_depth"] = save_image(f"{out_dir}/{name}_floodDepth.png", unit, "attention")
                for key in ("max_depth", "mean_depth", "volume"):
                    written[key] = res["depth"][key]
        elif "flood_logits" in res:
            written["flood_mask"] = save_image(f"{out_dir}/{name}_floodMask.png", res["flood_logits"], "mask_logits")
        if drainage:
            from .flow import render_flow
            unit = render_flow(res["flow"]["accumulation"])[None, None]
            written["flow_accumulation"] = save_image(f"{out_dir}/{name}_flowAccumulation.png", unit, "attention")
            written["pit_count"] = res["flow"]["pit_count"]
        if self.verbose:
            print(f"Saving the prediction of scene '{name}' to {written['prediction']}")
        self.last_scene = res
        return written

    def _sheet_columns(self, inputs, outputs, masks, targets):
        cols = [("Input", "rgb", inputs), ("Generator Output", "rgb", outputs)]
        if masks is not None:
            # the fixed 0..1 range of plot_image; the reference's plot_sample_images lets matplotlib autoscale
            cols.append(("Attention Mask", "attention", masks))
        return cols + [("Ground Truth Output", "rgb", targets)]

    def plot_sample_images(self, num_images, use_test_data):
        """models/model.py:542-596: one sheet per generator and split (training, validation[, test]) of the first
        num_images loader items (batch element 0 of each batch): input | output | [attention mask] | ground truth,
        with the reference's seeding (torch.manual_seed(self.seed) before each loader pass, torch.manual_seed(47)
        before each generator call), its input / output swap for the post-to-pre generator and its file names.  The
        generators run under torch.no_grad() in the mode they are in.  Returns the paths written."""
        import os

        from .render import save_sheet
        if self.model_is_cycle:
            generators = [("pre-to-post", self.pre_to_post_generator), ("post-to-pre", self.post_to_pre_generator)]
        else:
            generators = [("pre-to-post", self.generator)]
        splits, loaders = ["training", "validation"], [self.train_loader, self.val_loader]
        if use_test_data:
            splits, loaders = splits + ["test"], loaders + [self.test_loader]
        os.makedirs(f"{self.data_path}/images", exist_ok=True)
        paths = []
        for label, generator in generators:
            for split, loader in zip(splits, loaders):
                if loader is None:
                    raise RuntimeError(f"plot_sample_images: no {split} loader")
                xs, outs, masks, ys, names = [], [], [], [], []
                torch.manual_seed(self.seed)
                for i, (input_stack, output_image, image_name) in enumerate(loader):
                    input_stack = input_stack.to(self.device)
                    output_image = output_image.to(self.device)
                    if label == "post-to-pre":                                    # models/model.py:566-574
                        store_output = output_image
                        if self.topography:
                            output_image = input_stack[:, :3]
                            input_stack = torch.cat((store_output, input_stack[:, 3:]), dim=1)
                        else:
                            output_image, input_stack = input_stack, store_output
                    torch.manual_seed(47)
                    with torch.no_grad():
                        out = generator(input_stack)
                    xs.append(input_stack[:1])
                    outs.append(out[:1])
                    ys.append(output_image[:1])
                    if self.model_is_attention:
                        masks.append(generator.last_attention_mask[:1])
                    names.append(image_name[0])
                    if i >= num_images - 1:
                        break
                if not names:
                    raise RuntimeError(f"plot_sample_images: the {split} loader is empty")
                info = f"{split}{'_' + label if len(generators) > 1 else ''}"
                path = self.create_path("image", info=info)
                self.last_panels = save_sheet(path, self._sheet_columns(xs, outs, masks if self.model_is_attention
                                                                        else None, ys), names)
                if self.verbose:
                    print(f"Saving {split} {label + ' ' if len(generators) > 1 else ''}sample images to {path}")
                paths.append(path)
        return paths

    def checkpoint(self, epoch):
        if self.model_is_cycle:                                   # models/model.py:335-355 (cycle keys)
            ck = {"model": self.model, "starting_epoch": epoch + 1, "num_epochs": self.num_epochs,
                  "topography": self.topography, "all_losses": self.all_losses,
                  "add_identity_loss": self.add_identity_loss}
            for name in self._cycle_nets() + ["optimizer_generator", "optimizer_discriminator",
                                              "scheduler_generator", "scheduler_discriminator"]:
                ck[name] = getattr(self, name).state_dict()
            return ck
        return {"model": self.model, "starting_epoch": epoch + 1, "num_epochs": self.num_epochs,
                "topography": self.topography,
                "optimizer_generator": self.optimizer_generator.state_dict(),
                "optimizer_discriminator": self.optimizer_discriminator.state_dict(),
                "scheduler_generator": self.scheduler_generator.state_dict(),
                "scheduler_discriminator": self.scheduler_discriminator.state_dict(),
                "all_losses": self.all_losses, "add_identity_loss": self.add_identity_loss,
                "discriminator": self.discriminator.state_dict(), "generator": self.generator.state_dict()}
