"""Training loop of the general-CF scenario; same public surface as the reference's `Trainer`
(trainer/trainer.py:39-196): `create_optimizer`, `train_epoch`, `train` (optional early stop on
the first configured metric), `evaluate`, `test`, `save_model`, `load_model`; per step
zero_grad -> cal_loss -> backward -> step.  Of the eleven model-specific trainers upstream, AutoCF's, GFormer's and
AdaGCL's are here (`AutoCFTrainer`, `GFormerTrainer`, `AdaGCLTrainer`); the others belong to models outside this path."""
import os
import time
from copy import deepcopy

import numpy as np
import torch
import torch.optim as optim

from ..config.configurator import configs
from ..models.bulid_model import build_model
from .metrics import Metric
from .utils import DisabledSummaryWriter, log_exceptions

writer = DisabledSummaryWriter()


def init_seed():
    """Seed numpy (negative sampling), torch CPU (init, shuffling, augmentation draws) and the GPU
    generators when train.reproducible is set (reference :26-36)."""
    train_cfg = configs['train']
    if train_cfg.get('reproducible'):
        seed = train_cfg['seed']
        np.random.seed(seed)
        torch.manual_seed(seed)
        if torch.cuda.is_available():
            torch.cuda.manual_seed_all(seed)


class Trainer(object):
    def __init__(self, data_handler, logger):
        self.data_handler = data_handler
        self.logger = logger
        self.metric = Metric()

    def create_optimizer(self, model):
        cfg = configs['optimizer']
        if cfg['name'] == 'adam':
            # train.hip_graph replays the step from a captured hipGraph: the step counter must live on the device
            graphed = bool(configs['train'].get('hip_graph'))
            if cfg.get('fused'):        # one HIP pass per table, step counter on the device (sslrec_amd/optim.py)
                from ..optim import FusedAdam
                self.optimizer = FusedAdam(model.parameters(), lr=cfg['lr'], weight_decay=cfg['weight_decay'])
            else:
                self.optimizer = optim.Adam(model.parameters(), lr=cfg['lr'], weight_decay=cfg['weight_decay'],
                                            **({'capturable': True} if graphed else {}))
        else:
            raise NotImplementedError("optimizer '%s'" % cfg['name'])
        self._graph = None

    # ---- opt-in: one training step captured as a hipGraph (train.hip_graph: true) ------------------------
    # A LightGCN step is ~40 kernel launches of 5-100 us; issued from Python they take ~1.4 ms of wall time for
    # ~0.9 ms of GPU work.  The step (cal_loss, backward, Adam) is captured ONCE after a few eager warm-up steps
    # and replayed with the batch copied into static index tensors; losses are accumulated on the device and read
    # once per epoch.  Needs device-side augmentation RNG (model.device_rng) -- a host draw cannot be captured --
    # and full batches (the last, shorter batch of an epoch runs eagerly).
    def _backward(self, loss):
        """loss.backward() with d loss / d loss = 1 made once per device instead of filled by autograd on every step"""
        key = (loss.device, loss.dtype)
        one = self._ones.get(key) if hasattr(self, '_ones') else None
        if one is None:
            if not hasattr(self, '_ones'):
                self._ones = {}
            one = self._ones[key] = torch.ones((), dtype=loss.dtype, device=loss.device)
        loss.backward(one if loss.dim() == 0 else None)

    def _eager_step(self, model, batch_data):
        self.optimizer.zero_grad(set_to_none=True)
        loss, loss_dict = model.cal_loss(batch_data)
        self._backward(loss)
        self.optimizer.step()
        return loss, loss_dict

    @staticmethod
    def _device_of(model):
        """device of the model's parameters; a plugin that is not an nn.Module, or has no parameters, runs on the configured device"""
        try:
            return next(model.parameters()).device
        except (AttributeError, StopIteration, TypeError):
            return torch.device(configs['device'])

    @staticmethod
    def _host_rng_in_step(model):
        """True when the model's training forward draws from the CPU generator (the reference's EdgeDrop / EmbedPerturb
        behaviour, kept for bit parity unless model.device_rng is set): such a draw + H2D copy cannot be captured"""
        mcfg = configs['model']
        if mcfg.get('device_rng'):
            return False
        from ..rng import active_host_replay
        dev = Trainer._device_of(model)
        if active_host_replay(dev) is not None:
            return False         # the CPU generator's stream is produced by a kernel (sslrec_amd/csrc/mt19937.hip): capturable
        name = type(model).__name__.lower()
        return name in ('sgl', 'simgcl') or (name == 'lightgcn' and float(mcfg.get('keep_rate', 1.0)) != 1.0)

    def _capture_step(self, model, batch_data):
        if self._host_rng_in_step(model):
            raise RuntimeError('train.hip_graph needs device-side augmentation RNG: set model.device_rng (the CPU draws of '
                               'EdgeDrop / EmbedPerturb and their host-to-device copies cannot be captured in a hipGraph)')
        dev = batch_data[0].device
        static_batch = [b.clone() for b in batch_data]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            # warm-up (layouts, workspaces, optimizer state, LDS attributes) that must NOT advance the training:
            # parameters, moments and step counters are put back IN PLACE afterwards -- the captured graph holds
            # their addresses.  Optimizer state that did not exist before the warm-up goes back to zero.
            def opt_tensors():
                from ..rng import active_host_replay
                replay = active_host_replay(dev)
                if replay is not None:
                    replay.attach()                                  # its state is on the device before the snapshot is taken
                out = [replay.mt] if replay is not None else []      # the warm-up's draws must not advance the replayed generator
                out += list(getattr(self.optimizer, '_ticks', {}).values())
                for st in self.optimizer.state.values():
                    out += [v for v in st.values() if torch.is_tensor(v)]
                return out
            params = [p.data for p in model.parameters()]
            before = {id(t): t.clone() for t in params + opt_tensors()}
            for _ in range(3):
                self._eager_step(model, static_batch)
            for t in params + opt_tensors():
                if id(t) in before:
                    t.copy_(before[id(t)])
                else:
                    t.zero_()
        torch.cuda.current_stream(dev).wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        self.optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(graph):
            loss, loss_dict = model.cal_loss(static_batch)
            self._backward(loss)
            self.optimizer.step()
            outs = {'loss': loss.detach().float().reshape(())}
            for name, value in loss_dict.items():
                outs['part_' + name] = (value.detach() if torch.is_tensor(value) else torch.tensor(float(value), device=dev)).float().reshape(())
        return {'graph': graph, 'batch': static_batch, 'outs': outs, 'B': int(batch_data[0].shape[0])}

    def _train_epoch_graphed(self, model, epoch_idx):
        loader = self.data_handler.train_dataloader
        loader.dataset.sample_negs()
        dev = configs['device']
        model.train()
        sums, n_batches = {}, len(loader)

        def add(outs):
            for k, v in outs.items():
                sums[k] = sums[k] + v if k in sums else v.clone()

        from ..rng import active_host_replay
        replay = None if configs['model'].get('device_rng') else active_host_replay(self._device_of(model))
        attached = False
        for tem in loader:
            batch_data = [x.long().to(dev) for x in tem]
            st = self._graph
            if st is None and batch_data[0].shape[0] == configs['train']['batch_size']:
                st = self._graph = self._capture_step(model, batch_data)
                # the warm-up steps' effect on parameters and optimizer state was undone in place and capture executes
                # nothing: the replay below is this batch's one real step
            if st is not None and batch_data[0].shape[0] == st['B']:
                if replay is not None and not attached:
                    # a replay bypasses HostGeneratorReplay.rand()/keep_mask(): follow the host generator here if it moved
                    # since the last flush (the DataLoader's shuffle seed is drawn from it when the iterator is created),
                    # or raise if it moved while the device was ahead
                    replay.attach()
                    attached = True
                for dst, src in zip(st['batch'], batch_data):
                    dst.copy_(src)
                st['graph'].replay()
                if replay is not None:
                    replay.ahead = True      # the captured generator kernels advanced the device state: flush() must write it back
                add(st['outs'])
            else:
                loss, loss_dict = self._eager_step(model, batch_data)
                outs = {'loss': loss.detach().float().reshape(())}
                for name, value in loss_dict.items():
                    outs['part_' + name] = (value.detach() if torch.is_tensor(value) else torch.tensor(float(value), device=dev)).float().reshape(())
                add(outs)
        host = {k: float(v.item()) for k, v in sums.items()}              # one synchronisation per epoch
        steps = max(1, len(loader.dataset) // configs['train']['batch_size'])
        writer.add_scalar('Loss/train', host.get('loss', 0.0) / steps, epoch_idx)
        loss_log = {k[5:]: v / n_batches for k, v in host.items() if k.startswith('part_')}
        self.logger.log_loss(epoch_idx, loss_log, save_to_log=bool(configs['train']['log_loss']))

    def train_epoch(self, model, epoch_idx):
        try:
            if configs['train'].get('hip_graph'):
                return self._train_epoch_graphed(model, epoch_idx)
            return self._train_epoch_eager(model, epoch_idx)
        finally:
            # parity-mode draws are produced on the device (sslrec_amd.rng.HostGeneratorReplay): hand the generator back to
            # the host before anything there draws again (next epoch's shuffling, evaluation, model construction)
            from ..rng import flush_host_replay
            flush_host_replay()

    def _epoch_extras(self, model):
        """what a trainer appends to every batch of the epoch that starts (KGCLTrainer: the epoch's augmented views); nothing here"""
        return []

    def _train_epoch_eager(self, model, epoch_idx):
        """reference trainer/trainer.py:51-84.  The reference reads `loss.item()` (and every logged part) in every step: three device
        synchronisations per step, during which the host cannot queue the next step's launches.  Here the step's 0-d tensors are kept and
        read ONCE at the end of the epoch; the sums are then formed on the host in the reference's order and arithmetic (Python floats,
        `value / n_batches` per step), so the logged numbers are the same -- only their moment of transfer moved."""
        loader = self.data_handler.train_dataloader
        loader.dataset.sample_negs()
        n_batches = len(loader)
        model.train()
        extras = self._epoch_extras(model)
        kept, names = [], None
        for tem in loader:
            self.optimizer.zero_grad()
            batch_data = [x.long().to(configs['device']) for x in tem] + extras
            loss, loss_dict = model.cal_loss(batch_data)
            self._backward(loss)
            self.optimizer.step()
            if names is None:
                names = list(loss_dict)
            dev = loss.device
            kept.append([loss.detach().reshape(())] + [(loss_dict[k].detach().reshape(()).to(loss.dtype) if torch.is_tensor(loss_dict[k])
                                                        else torch.tensor(float(loss_dict[k]), dtype=loss.dtype, device=dev)) for k in names])
        loss_log, ep_loss = {}, 0.0
        if kept:
            host = torch.stack([torch.stack(row) for row in kept]).double().cpu().tolist()      # one synchronisation per epoch
            for row in host:
                ep_loss += row[0]
                for name, value in zip(names, row[1:]):
                    loss_log[name] = loss_log.get(name, 0.0) + value / n_batches
        steps = max(1, len(loader.dataset) // configs['train']['batch_size'])
        writer.add_scalar('Loss/train', ep_loss / steps, epoch_idx)
        self.logger.log_loss(epoch_idx, loss_log, save_to_log=bool(configs['train']['log_loss']))

    @log_exceptions
    def train(self, model):
        from .. import rng
        dev = self._device_of(model)
        # train.host_rng_replay (default on): the reference's CPU draws for EdgeDrop / EmbedPerturb come out of the same
        # generator algorithm running on the GPU -- same numbers, no host stall; flushed back at every epoch boundary
        replay = dev.type == 'cuda' and configs['train'].get('host_rng_replay', True) and not configs['model'].get('device_rng')
        mine = replay and rng.active_host_replay(dev) is None      # a replay the caller enabled stays the caller's
        rep, ahead_before = None, None
        if replay:
            rep = rng.enable_host_replay(dev)
            ahead_before = rep.draw_ahead
            if configs['train'].get('hip_graph'):      # a captured step generates its numbers inside the graph: nothing to draw ahead
                rep.draw_ahead = False
        try:
            return self._train(model)
        finally:
            if mine:
                rng.disable_host_replay(dev)
            elif replay:
                rep.draw_ahead = ahead_before          # the caller's replay goes back as it came
                rng.flush_host_replay()

    def _train(self, model):
        self.create_optimizer(model)
        cfg = configs['train']
        if not cfg['early_stop']:
            for epoch_idx in range(cfg['epoch']):
                self.train_epoch(model, epoch_idx)
                if epoch_idx % cfg['test_step'] == 0:
                    self.evaluate(model, epoch_idx)
            self.test(model)
            self.save_model(model)
            return model
        patience, best_epoch, best_metric, best_state = 0, 0, -1e9, None
        first_metric = configs['test']['metrics'][0]
        for epoch_idx in range(cfg['epoch']):
            self.train_epoch(model, epoch_idx)
            if epoch_idx % cfg['test_step'] == 0:
                score = self.evaluate(model, epoch_idx)[first_metric][0]
                if score > best_metric:
                    patience, best_epoch, best_metric = 0, epoch_idx, score
                    best_state = deepcopy(model.state_dict())
                    self.logger.log('Validation score increased.  Copying the best model ...')
                else:
                    patience += 1
                    self.logger.log('Early stop counter: {} out of {}'.format(patience, cfg['patience']))
                if patience == cfg['patience']:
                    break
        self.logger.log('Best Epoch {}'.format(best_epoch))
        model = build_model(self.data_handler).to(configs['device'])
        if best_state is not None:
            model.load_state_dict(best_state)
        self.evaluate(model)
        self.test(model)
        self.save_model(model)
        return model

    @log_exceptions
    def evaluate(self, model, epoch_idx=None):
        model.eval()
        if hasattr(self.data_handler, 'valid_dataloader'):
            loader, name = self.data_handler.valid_dataloader, 'Validation set'
        elif hasattr(self.data_handler, 'test_dataloader'):
            loader, name = self.data_handler.test_dataloader, 'Test set'
        else:
            raise NotImplementedError
        result = self.metric.eval(model, loader)
        self.logger.log_eval(result, configs['test']['k'], data_type=name, epoch_idx=epoch_idx)
        return result

    @log_exceptions
    def test(self, model):
        model.eval()
        if not hasattr(self.data_handler, 'test_dataloader'):
            raise NotImplementedError
        result = self.metric.eval(model, self.data_handler.test_dataloader)
        self.logger.log_eval(result, configs['test']['k'], data_type='Test set')
        return result

    def save_model(self, model):
        if not configs['train']['save_model']:
            return
        name, data = configs['model']['name'], configs['data']['name']
        if configs['tune']['enable']:
            directory, tag = './checkpoint/{}/tune'.format(name), configs['tune']['now_para_str']
        else:
            directory, tag = './checkpoint/{}'.format(name), int(time.time())
        os.makedirs(directory, exist_ok=True)
        path = '{}/{}-{}-{}.pth'.format(directory, name, data, tag)
        torch.save(model.state_dict(), path)
        self.logger.log('Save model parameters to {}'.format(path))

    def load_model(self, model):
        if 'pretrain_path' not in configs['train']:
            raise KeyError("No pretrain_path in configs['train']")
        path = configs['train']['pretrain_path']
        model.load_state_dict(torch.load(path))
        self.logger.log('Load model parameters from {}'.format(path))
        return model


class AutoCFTrainer(Trainer):
    """reference trainer/trainer.py:201-250: every `model.fix_steps` steps the model samples seeds (`sample_subgraphs`) and masks their
    subgraphs (`mask_subgraphs`); those steps add -sampScores.mean() as `infomax_loss`.  The batches come from the default stream.
    As in `_train_epoch_eager`, the step's 0-d tensors are read once at the end of the epoch and summed on the host in the
    reference's order.  train.hip_graph is refused: the resampling steps draw on the host and build a new graph, which a captured
    step cannot do.  train.host_rng_replay is OFF for this trainer: the model's draws (t.rand / t.randint in LocalGraph and the
    masker) go to the CPU generator directly, which the replay would have to hand back around every resampling."""

    def __init__(self, data_handler, logger):
        super().__init__(data_handler, logger)
        self.fix_steps = configs['model']['fix_steps']
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by AutoCFTrainer: every model.fix_steps steps the step draws on '
                                      'the host and rebuilds its graphs')

    @log_exceptions
    def train(self, model):
        from .. import rng
        if rng.active_host_replay(self._device_of(model)) is not None:
            raise RuntimeError('AutoCFTrainer draws from the CPU generator directly: disable the host generator replay '
                               '(train.host_rng_replay) before training AutoCF')
        return self._train(model)

    def train_epoch(self, model, epoch_idx):
        loader = self.data_handler.train_dataloader
        loader.dataset.sample_negs()
        n_batches = len(loader)
        model.train()
        kept = []
        encoder_adj = decoder_adj = None
        for i, tem in enumerate(loader):
            self.optimizer.zero_grad()
            batch_data = [x.long().to(configs['device']) for x in tem]
            resample = i % self.fix_steps == 0
            if resample:
                samp_scores, seeds = model.sample_subgraphs()
                encoder_adj, decoder_adj = model.mask_subgraphs(seeds)
            loss, loss_dict = model.cal_loss(batch_data, encoder_adj, decoder_adj)
            if resample:
                infomax = -samp_scores.mean()
                loss = loss + infomax
                loss_dict['infomax_loss'] = infomax
            self._backward(loss)
            self.optimizer.step()
            kept.append((loss.detach().reshape(()), {k: (v.detach().reshape(()).to(loss.dtype) if torch.is_tensor(v)
                                                         else torch.tensor(float(v), dtype=loss.dtype, device=loss.device))
                                                     for k, v in loss_dict.items()}))
        loss_log, ep_loss = {}, 0.0
        if kept:
            flat = torch.stack([x for loss, parts in kept for x in [loss] + list(parts.values())]).double().cpu().tolist()      # one synchronisation per epoch
            pos = 0
            for _, parts in kept:
                ep_loss += flat[pos]
                for j, name in enumerate(parts):
                    loss_log[name] = loss_log.get(name, 0.0) + flat[pos + 1 + j] / n_batches
                pos += 1 + len(parts)
        self.step_losses = [sorted(parts) for _, parts in kept]          # names logged by every step of the last epoch
        steps = max(1, len(loader.dataset) // configs['train']['batch_size'])
        writer.add_scalar('Loss/train', ep_loss / steps, epoch_idx)
        self.logger.log_loss(epoch_idx, loss_log, save_to_log=bool(configs['train']['log_loss']))


class GFormerTrainer(Trainer):
    """reference trainer/trainer.py:253-296: `sample_negs`, then `model.preSelect_anchor_set()` once per epoch; every
    `model.fix_steps` steps `model.localGraph` scores the entries of a widened adjacency and `model.masker` draws the encoder / decoder /
    sub / cmp graphs from them; every step is cal_loss -> zero_grad -> backward -> step.  All draws of the epoch are numpy's global
    generator, in the reference's order: the negative sampler's, the anchors', the masker's.  As in `_train_epoch_eager`, the step's 0-d
    tensors are read once at the end of the epoch and summed on the host in the reference's order.  train.hip_graph is refused: the
    resampling steps draw on the host and build new graphs, which a captured step cannot do.  The model makes no torch draw while
    training, so the host generator replay is not switched on for this trainer."""

    def __init__(self, data_handler, logger):
        super().__init__(data_handler, logger)
        self.handler = data_handler
        self.user = configs['data']['user_num']
        self.item = configs['data']['item_num']
        self.latdim = configs['model']['embedding_size']
        self.fixSteps = configs['model']['fix_steps']
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by GFormerTrainer: every model.fix_steps steps the step draws on '
                                      'the host and rebuilds its graphs')

    @log_exceptions
    def train(self, model):
        return self._train(model)

    def train_epoch(self, model, epoch_idx):
        model.train()
        loader = self.data_handler.train_dataloader
        loader.dataset.sample_negs()
        model.preSelect_anchor_set()
        n_batches = len(loader)
        kept = []
        self.resampled_steps = []
        encoderAdj = decoderAdj = sub = cmp = None
        for i, tem in enumerate(loader):
            batch_data = [x.long().to(configs['device']) for x in tem]
            if i % self.fixSteps == 0:
                att_edge, add_adj = model.localGraph(self.handler.torch_adj, model.getEgoEmbeds(), self.handler)
                encoderAdj, decoderAdj, sub, cmp = model.masker(add_adj, att_edge)
                self.resampled_steps.append(i)
            loss, loss_dict = model.cal_loss(batch_data, encoderAdj, decoderAdj, sub, cmp)
            self.optimizer.zero_grad()
            self._backward(loss)
            self.optimizer.step()
            kept.append((loss.detach().reshape(()), {k: (v.detach().reshape(()).to(loss.dtype) if torch.is_tensor(v)
                                                         else torch.tensor(float(v), dtype=loss.dtype, device=loss.device))
                                                     for k, v in loss_dict.items()}))
        loss_log, ep_loss = {}, 0.0
        if kept:
            flat = torch.stack([x for loss, parts in kept for x in [loss] + list(parts.values())]).double().cpu().tolist()      # one synchronisation per epoch
            pos = 0
            for _, parts in kept:
                ep_loss += flat[pos]
                for j, name in enumerate(parts):
                    loss_log[name] = loss_log.get(name, 0.0) + flat[pos + 1 + j] / n_batches
                pos += 1 + len(parts)
        self.step_losses = [sorted(parts) for _, parts in kept]          # names logged by every step of the last epoch
        steps = max(1, len(loader.dataset) // configs['train']['batch_size'])
        writer.add_scalar('Loss/train', ep_loss / steps, epoch_idx)
        self.logger.log_loss(epoch_idx, loss_log, save_to_log=bool(configs['train']['log_loss']))


class KGCLTrainer(Trainer):
    """reference trainer/trainer.py:495-575 without its `train_trans` half: `Trainer.train_epoch` with `model.get_aug_views()` called once
    per epoch, after the negatives are sampled and before the batch loop, and the four views appended to every batch (:517-521).  One
    optimizer: upstream's second one, `kgtrans_optimizer`, only steps under `train_trans`, which the kg data handler refuses."""

    def _epoch_extras(self, model):
        return list(model.get_aug_views())


class AdaGCLTrainer(Trainer):
    """reference trainer/trainer.py:1114-1203: two view generators beside the model (`generator_1` a VGAE, `generator_2` a DenoiseNet),
    three Adam optimizers, and a step of four phases in the reference's order -- the contrastive loss of the two generated views, the
    information-bottleneck loss against that phase's outputs, the main BPR loss, then both generators' losses -- with the optimizer
    steps and zero-grads where the reference has them (:1153-1186).  The gate temperature follows
    max(0.05, init_temperature * temperature_decay^epoch) (:1157).  As in `_train_epoch_eager`, the step's 0-d tensors are read once
    at the end of the epoch and summed on the host in the reference's order; a generated view that kept no entry is reported there.
    train.hip_graph is refused: the step draws on the host (numpy's generator for the gate noise) and steps three optimizers between
    its backward passes.  train.host_rng_replay is OFF for this trainer, as for AutoCFTrainer: VGAE's t.randn goes to the CPU
    generator directly."""

    def __init__(self, data_handler, logger):
        from ..models.general_cf.adagcl import VGAE, DenoiseNet
        super().__init__(data_handler, logger)
        if configs['train'].get('hip_graph'):
            raise NotImplementedError('train.hip_graph is not supported by AdaGCLTrainer: every step draws the gate noise on the host and '
                                      'steps three optimizers between its backward passes')
        self.generator_1 = VGAE().to(configs['device'])
        self.generator_2 = DenoiseNet().to(configs['device'])

    def create_optimizer(self, model):
        self.generator_1.set_adagcl(model)
        self.generator_2.set_adagcl(model)
        model.set_denoiseNet(self.generator_2)
        cfg = configs['optimizer']
        if cfg['name'] != 'adam':
            raise NotImplementedError("optimizer '%s'" % cfg['name'])
        self.optimizer = optim.Adam(model.parameters(), lr=cfg['lr'], weight_decay=cfg['weight_decay'])
        self.optimizer_gen_1 = optim.Adam(self.generator_1.parameters(), lr=cfg['lr'], weight_decay=cfg['weight_decay'])
        self.optimizer_gen_2 = optim.Adam(filter(lambda p: p.requires_grad, self.generator_2.parameters()), lr=cfg['lr'],
                                          weight_decay=cfg['weight_decay'])
        self._graph = None

    @log_exceptions
    def train(self, model):
        from .. import rng
        if rng.active_host_replay(self._device_of(model)) is not None:
            raise RuntimeError('AdaGCLTrainer draws from the CPU generators directly: disable the host generator replay '
                               '(train.host_rng_replay) before training AdaGCL')
        return self._train(model)

    def generator_generate(self, generator):
        with torch.no_grad():
            return generator.vgae_generate(self.data_handler.torch_adj)

    @staticmethod
    def temperature(epoch_idx):
        m = configs['model']
        return max(0.05, m['init_temperature'] * pow(m['temperature_decay'], epoch_idx))

    def train_step(self, model, batch_data, temperature, probe=None):
        """one step (:1153-1188): (the four phase losses, the merged loss dictionary).  probe(name), if given, is called before the
        optimizer steps that end the phases 'cl', 'ib' and 'main' (tests read the gradients there)."""
        self.optimizer.zero_grad()
        self.optimizer_gen_1.zero_grad()
        self.optimizer_gen_2.zero_grad()
        model._begin_step()
        data1 = self.generator_generate(self.generator_1)

        loss_cl, loss_dict_cl, out1, out2 = model.cal_loss_cl(batch_data, data1)
        self._backward(loss_cl)
        if probe is not None:
            probe('cl')
        self.optimizer.step()
        self.optimizer.zero_grad()

        loss_ib, loss_dict_ib = model.cal_loss_ib(batch_data, data1, out1, out2)
        self._backward(loss_ib)
        if probe is not None:
            probe('ib')
        self.optimizer.step()
        self.optimizer.zero_grad()

        loss_main, loss_dict_main = model.cal_loss(batch_data)
        self._backward(loss_main)
        loss_vgae, loss_dict_vgae = self.generator_1.cal_loss_vgae(self.data_handler.torch_adj, batch_data)
        loss_denoise, loss_dict_denoise = self.generator_2.cal_loss_denoise(batch_data, temperature)
        loss_generator = loss_vgae + loss_denoise
        self._backward(loss_generator)
        if probe is not None:
            probe('main')
        self.optimizer.step()
        self.optimizer_gen_1.step()
        self.optimizer_gen_2.step()
        loss_dict = {**loss_dict_cl, **loss_dict_ib, **loss_dict_main, **loss_dict_vgae, **loss_dict_denoise}
        return (loss_cl, loss_ib, loss_main, loss_generator), loss_dict

    def train_epoch(self, model, epoch_idx):
        from ..models.general_cf.adagcl import check_kept
        loader = self.data_handler.train_dataloader
        loader.dataset.sample_negs()
        n_batches = len(loader)
        model.train()
        temperature = self.temperature(epoch_idx)
        kept, names, views = [], None, []
        for tem in loader:
            batch_data = [x.long().to(configs['device']) for x in tem]
            losses, loss_dict = self.train_step(model, batch_data, temperature)
            if names is None:
                names = list(loss_dict)
            views.append(self.generator_1.last['kept'])
            kept.append([x.detach().reshape(()).float() for x in losses] + [loss_dict[k].detach().reshape(()).float() for k in names])
        loss_log, ep_loss = {}, 0.0
        if kept:
            check_kept(torch.cat(views))                                                          # the epoch's one synchronisation ...
            host = torch.stack([torch.stack(row) for row in kept]).double().cpu().tolist()      # ... and its one transfer
            for row in host:
                ep_loss += sum(row[:4])
                for name, value in zip(names, row[4:]):
                    loss_log[name] = loss_log.get(name, 0.0) + value / n_batches
        steps = max(1, len(loader.dataset) // configs['train']['batch_size'])
        writer.add_scalar('Loss/train', ep_loss / steps, epoch_idx)
        self.loss_log = loss_log
        self.logger.log_loss(epoch_idx, loss_log, save_to_log=bool(configs['train']['log_loss']))
