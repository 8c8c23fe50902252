"""The optimizer steps of AgentPPO.update_net on the fused HIP gradient path (ops.FusedPPOGrad), as one object per
(FusedPPOGrad, buf_len, batch_size): `fused.static`.

Per optimizer step: indices -> minibatch r_sum scale -> three HIP launches (critic, actor, slab reduction) that leave
d(obj_united)/d(theta) in the flat gradient buffer.  On one GPU the reduction also applies Adam and writes the new parameter values
into the packed weight images (pime_ppo_minibatch_step + image map): nothing else is launched.  Under data parallelism ONE all-reduce
of the flat buffer follows, then the Adam launch (which keeps the images current as well).

The launch sequence of a step is identical every time, so after one eager step (which also creates Adam's state) it is captured into
HIP graphs and replayed (the update is otherwise bound by ~200 us/step of host work).  `StepForm` says which sequence that is;
DESIGN.md ("HIP graphs") has the table of forms.  A captured graph bakes in the tensors of this object, the step form and `baked`
(the data pointers of the update's states / actions, the loss scalars, the optimizer object and its learning rate); the
whole-update graph also n_steps.  When any of them changes, or the index table is re-allocated, `invalidate` drops the graphs."""
import functools
import weakref
from typing import NamedTuple

import torch

from . import graphs
from ..native import PimeError
from ..ops import FlatAdam


class StepForm(NamedTuple):
    """How one optimizer step is launched."""
    use_table: bool   # indices: all minibatches of the update drawn at once into a table the kernels walk with a device-side row
    #                   cursor (else an index hook hands over one tensor per step: host work in front of every step)
    one_graph: bool   # [gradients (, all-reduce), Adam] captured as ONE graph per step, and then the whole update as one graph
    #                   (else two graphs per step, [gradients] and [Adam], with the host work in between)
    fuse_adam: bool   # Adam rides in the gradient call's last launch (the slab reduction; pime_ppo_minibatch_step)
    dp_union: bool    # data parallel: the critic scale is that of the UNION minibatch, applied by the Adam launch


def step_form(agent, fused):
    """(StepForm, images_follow) from the agent's switches and what the probes found (None: not probed yet, taken as yes)."""
    dp, flat_adam = agent.dp, isinstance(agent.optimizer, FlatAdam)
    use_table = agent.index_hook is None
    # Data parallel: the flat-gradient all-reduce is an RCCL kernel on the compute stream, so it is captured between the gradient
    # launches and Adam like any other launch: ONE graph per optimizer step there too (the two-graph sequence with an eager
    # all-reduce in between cost 14 % on one rank before any communication).
    one_graph = (dp is None or graphs.collective_in_graph(agent)) and use_table and agent.launch_timer is None
    # Single GPU: the Adam step rides in the gradient call's last launch.  Data parallel (the all-reduce sits between gradients and
    # Adam), the bench's gradient-only event bracket, a torch optimizer, or nets on the split pipeline keep the separate Adam launch.
    fuse_adam = dp is None and agent.launch_timer is None and flat_adam and fused.adam_fusable is not False
    # Data parallel: the critic's gradient leaves the kernels UNSCALED with the minibatch's target moments behind it; the one
    # all-reduce of an optimizer step carries both, and the Adam launch applies 1 / (std of the UNION minibatch + 1e-5)
    # (agent.py:652 on the minibatch the ranks hold together).  Nets whose critic takes the split pipeline (a modular actor on a
    # stacked observation) keep the rank-local scale.
    dp_union = dp is not None and flat_adam and fused.dp_union_ok is not False
    # With the image map the launch that applies Adam writes every new parameter value into the packed images as well (the fused
    # step on one GPU, pime_adam_step_images behind the all-reduce under data parallelism): no re-pack launch.
    return StepForm(use_table, one_graph, fuse_adam, dp_union), flat_adam and fused.images_follow_step


def drop(fused):
    """A rebuilt optimizer: the captured graphs replay the OLD optimizer's buffers, and the new one has not stepped yet.  The next
    update starts from a new object, whose first step runs eagerly."""
    fused.static = None


class FusedPPOUpdate:
    def __init__(self, fused, buf_len, batch_size, state_dim, dev):
        """Tensors with stable addresses that the captured graphs read (the per-update r_sum / log-prob / advantage buffers are
        fresh allocations, so they are copied in)."""
        f32 = dict(dtype=torch.float32, device=dev)
        self.fused, self.buf_len, self.batch, self.dev = fused, buf_len, batch_size, dev
        self.r_sum, self.logprob, self.adv = (torch.empty(buf_len, **f32) for _ in range(3))
        self.action, self.state = torch.empty(buf_len, **f32), torch.empty((buf_len, state_dim), **f32)
        self.scale, self.last = torch.ones(1, **f32), torch.zeros(6, **f32)
        self.idx = torch.zeros(batch_size, dtype=torch.int64, device=dev)
        self.row = torch.zeros(1, dtype=torch.int64, device=dev)
        self.table = None
        self.warm = False          # one eager step has run
        self.agent = self.src = None   # of the running update: the agent and the (states, actions) the kernels read
        self.form = self.images_follow = self.baked = None
        self.invalidate()

    @classmethod
    def of(cls, fused, buf_len, batch_size, state_dim, dev):
        st = fused.static
        if st is None or (st.buf_len, st.batch) != (buf_len, batch_size):
            st = fused.static = cls(fused, buf_len, batch_size, state_dim, dev)
        return st

    @property
    def key(self):
        """Everything the captured graphs bake in besides this object's tensors."""
        return self.baked, self.form

    def invalidate(self):
        self.graph_a = self.graph_b = self.graph_full = self.graph_update = None
        self.graph_update_steps = None   # the n_steps the whole-update graph was captured (or refused) for

    # ---- one update: load, then run ----------------------------------------------------------------------
    def load(self, agent, n_steps, buf_state, buf_action, buf_r_sum, buf_logprob, buf_advantage):
        """The update's buffers and minibatch indices to where the kernels read them; settles the step form and the cache key."""
        # (a proxy: agent._packed -> fused -> static -> agent would be a reference cycle, and the agent's tensors and graphs would
        # then be freed only by the cyclic collector)
        self.agent, cached = weakref.proxy(agent), self.key
        self.r_sum.copy_(buf_r_sum); self.logprob.copy_(buf_logprob); self.adv.copy_(buf_advantage)
        # states / actions: the trajectory buffer's storage is already contiguous and address-stable; a flat ring
        # buffer hands out strided column views, which are copied once per update
        action = buf_action.reshape(-1)
        if not (action.is_contiguous() and buf_state.is_contiguous()):
            self.action.copy_(action); self.state.copy_(buf_state)
            action, buf_state = self.action, self.state
        self.src = buf_state, action
        form, self.images_follow = step_form(agent, self.fused)
        if form.use_table:
            self._fill_table(n_steps)
        self.form = self._probed(form)
        # data pointers, the loss scalars (launch arguments) and the optimizer object whose buffers and learning rate the Adam
        # launch reads
        self.baked = (buf_state.data_ptr(), action.data_ptr(), float(agent.ratio_clip), float(agent.lambda_entropy),
                      id(agent.optimizer), float(getattr(agent.optimizer, "lr", agent.learning_rate)))
        if self.key != cached:
            self.invalidate()

    def _fill_table(self, n_steps):
        """With torch's own draw, all n_steps minibatches are drawn at once (agent.py:630 draws them one torch.randint per step), so
        a captured graph needs no per-step input."""
        agent = self.agent
        if self.table is None or self.table.shape[0] < n_steps:
            self.table = torch.empty((n_steps, self.batch), dtype=torch.int64, device=self.dev)
            self.invalidate()
        if agent.index_table_hook is not None:
            self.table[:n_steps].copy_(agent.index_table_hook(n_steps, self.buf_len, self.batch).to(self.dev))
        else:
            torch.randint(self.buf_len, size=(n_steps, self.batch), device=self.dev, out=self.table[:n_steps])
        self.row.zero_()

    def _probed(self, form):
        """`form` after asking the library, once per FusedPPOGrad, whether it serves these nets in that form."""
        fused, opt = self.fused, self.agent.optimizer
        self.form = form   # (the probes launch grads() in it)
        if form.dp_union and fused.dp_union_ok is None:     # does the library defer the scale for these nets?
            fused.dp_union_ok = self._probe((fused.loss_sums, self.row), lambda exc: print(
                f"| critic scale over the union minibatch unavailable for these nets ({exc}); using the rank-local scale"))
        if form.fuse_adam and fused.adam_fusable is None:   # does the library fuse the step for these nets?
            fused.adam_fusable = self._probe((fused.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.step_count, fused.loss_sums,
                                              self.row), lambda exc: None)
            if self.images_follow:
                fused.repack()   # ... nor in the packed images it may have updated
        return step_form(self.agent, fused)[0]

    def _probe(self, restore, on_refusal):
        """Does the library run grads() in self.form?  The probe must leave no trace: `restore` are the tensors it writes."""
        snap = [t.clone() for t in restore]
        served = True
        try:
            self.grads()
        except PimeError as exc:
            on_refusal(exc)
            served = False
        for dst, src in zip(restore, snap):
            dst.copy_(src)
        return served

    # ---- the launches of one optimizer step --------------------------------------------------------------
    def grads(self):   # overwrite: no zeroing launch; the running sum of the critic scale lands in loss_sums[3]
        agent, form, (state, action) = self.agent, self.form, self.src
        self.fused(state, action, self.logprob, self.adv, self.r_sum, self.table if form.use_table else self.idx, agent.ratio_clip,
                   agent.lambda_entropy, self.scale, overwrite=True, index_row=self.row if form.use_table else None,
                   adam=agent.optimizer if form.fuse_adam else None, defer_critic_scale=form.dp_union)

    def all_reduce(self):
        self.agent.dp.all_reduce_mean(self.fused.flat_grad_dp if self.form.dp_union else self.fused.flat_grad)

    def apply(self):
        agent, fused = self.agent, self.fused
        if not self.form.fuse_adam:
            if self.form.dp_union:
                agent.optimizer.step(images=fused if self.images_follow else None, dp=(fused, agent.dp.world))
            elif self.images_follow:
                agent.optimizer.step(images=fused)
            else:
                agent.optimizer.step()
        if not self.images_follow:
            fused.repack()

    def whole_update(self, n_steps):
        """n_steps x (critic, actor, reduction [, all-reduce, Adam]) and the copy of the loss sums in front of the last step."""
        for k in range(n_steps):
            if k == n_steps - 1:
                self.last.copy_(self.fused.loss_sums)
            self.grads()
            if self.agent.dp is not None:
                self.all_reduce()
            self.apply()

    # ---- capture and replay ------------------------------------------------------------------------------
    def run(self, n_steps):
        """All optimizer steps of the update: the whole-update graph, or per step the captured graph(s), or eager launches.  Returns
        the loss sums in front of the last step (None if n_steps == 0)."""
        agent, fused = self.agent, self.fused
        # With the index table every optimizer step is the same launch sequence (the row cursor lives on the device), so once the
        # per-step graph exists the WHOLE update is captured as one graph: one replay per update_net instead of n_steps, and the
        # ~5 us between two replays become a node boundary.
        if (agent.use_update_graph and self.form.one_graph and agent.use_hip_graphs and self.graph_full is not None and n_steps > 1
                and self.graph_update_steps != n_steps):
            self._capture_whole_update(n_steps)
        last = None
        if self.graph_update is not None and self.graph_update_steps == n_steps and self.form.one_graph and agent.use_update_graph:
            self.graph_update.replay()
            last = self.last.clone()
            n_steps = 0
        for step in range(n_steps):
            if not self.form.use_table:
                self.idx.copy_(agent.index_hook(step, self.buf_len, self.batch).to(self.dev))
            if step == n_steps - 1:
                last = fused.loss_sums.clone()
            if agent.use_hip_graphs and self.warm and self.graph_a is None and self.graph_full is None:
                self._capture_step()
            self._step()
        self.src = None   # (a widened copy of binary16 rows is freed here, as every update's temporaries are)
        return last

    def _capture_whole_update(self, n_steps):
        self.graph_update, self.graph_update_steps = None, n_steps
        try:
            self.graph_update = graphs.capture(self.dev, functools.partial(self.whole_update, n_steps))
        except RuntimeError as exc:
            print(f"| capture of the whole update refused ({exc}); replaying one graph per optimizer step")
            self.agent.use_update_graph = False
            torch.cuda.synchronize(self.dev)

    def _capture_step(self):
        agent, form, dev = self.agent, self.form, self.dev
        try:
            if form.one_graph and agent.dp is not None:
                # If the capture fails (a torch / RCCL build that refuses collectives under capture) the agent falls back to the
                # two-graph sequence for good.
                self.graph_full, refused = graphs.capture_on_every_rank(agent.dp, dev, self.grads, self.all_reduce, self.apply)
                if self.graph_full is None:
                    print(f"| all-reduce inside the HIP graph refused on a rank ({refused}); every rank uses the "
                          "two-graph step sequence")
                    agent.use_graph_collective = False
                    self.form = form._replace(one_graph=False)
                    self.graph_a, self.graph_b = graphs.capture(dev, self.grads), graphs.capture(dev, self.apply)
            elif form.one_graph:
                self.graph_full = graphs.capture(dev, self.grads, self.apply)
            else:
                self.graph_a = graphs.capture(dev, self.grads)
                # nothing left to launch after a fused step that keeps the images current
                self.graph_b = None if (self.images_follow and form.fuse_adam) else graphs.capture(dev, self.apply)
        except RuntimeError as exc:  # keep training on the eager launch sequence
            print(f"| HIP graph capture failed ({exc}); continuing with eager launches")
            agent.use_hip_graphs = False
            torch.cuda.synchronize(dev)

    def _step(self):
        agent = self.agent
        if self.graph_full is not None:
            self.graph_full.replay()
            return
        run = self.graph_a.replay if self.graph_a is not None else self.grads
        if agent.launch_timer is not None:   # bench.py: HIP events around the gradient launches only
            agent.launch_timer("ppo_minibatch_grad", run)
        else:
            run()
        if agent.dp is not None:
            self.all_reduce()
        if self.graph_b is not None:
            self.graph_b.replay()
        else:
            self.apply()
            self.warm = True
