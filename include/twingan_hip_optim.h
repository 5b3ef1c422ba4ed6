/* The reference's --optimizer choices besides Adam as further rules of Adam's fused apply kernel (apply_kernel<RULE, VEC, EMA>,
 * twingan_amd/csrc/reduce.hip; Adam's entry points tg_adam_* are in twingan_hip.h), same library and conventions as twingan_hip.h: int-returning entry points, TG_OK or a TG_E* code with the text in tg_last_error(), every
 * launch enqueued on `stream` without host synchronisation. */
#ifndef TWINGAN_HIP_OPTIM_H_
#define TWINGAN_HIP_OPTIM_H_

#include "twingan_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* --optimizer (model/model_inheritor.py:516-565 _configure_optimizer).  Adam keeps its own entry points (tg_adam_*). */
enum {
  TG_OPT_SGD = 0,      /* tf.train.GradientDescentOptimizer        model_inheritor.py:561-562 */
  TG_OPT_MOMENTUM = 1, /* tf.train.MomentumOptimizer               :550-554 (use_nesterov unset) */
  TG_OPT_ADAGRAD = 2,  /* tf.train.AdagradOptimizer                :533-536 */
  TG_OPT_RMSPROP = 3,  /* tf.train.RMSPropOptimizer                :555-560 (centered unset) */
  TG_OPT_ADADELTA = 4, /* tf.train.AdadeltaOptimizer               :528-532 */
  TG_OPT_FTRL = 5      /* tf.train.FtrlOptimizer                   :543-549 (l2_shrinkage unset) */
};

/* The hyper-parameters of every rule, by value (a captured graph replays them); a rule reads the fields it names:
 *   sgd       lr                                       theta -= lr g
 *   momentum  lr, momentum                             a = momentum a + g; theta -= lr a
 *   adagrad   lr                                       a += g^2; theta -= lr g / sqrt(a)
 *   rmsprop   lr, decay_or_rho, momentum, eps          ms += (g^2 - ms)(1 - decay); mom = momentum mom + lr g / sqrt(ms + eps);
 *                                                      theta -= mom
 *   adadelta  lr, decay_or_rho, eps                    accum = rho accum + (1 - rho) g^2; u = sqrt(upd + eps) / sqrt(accum + eps) g;
 *                                                      theta -= lr u; upd = rho upd + (1 - rho) u^2
 *   ftrl      lr, lr_power (<= 0), l1, l2              n = accum + g^2; sigma = (n^-p - accum^-p) / lr; linear += g - sigma theta;
 *                                                      q = n^-p / lr + 2 l2; theta = |linear| > l1 ? (sign(linear) l1 - linear) / q : 0;
 *                                                      accum = n      (p = lr_power; -0.5 takes sqrt)
 * TF 1.8 core/kernels/training_ops.cc, the dense functors. */
typedef struct TgOptimHyper {
  float lr, momentum, decay_or_rho, eps, lr_power, l1, l2;
} TgOptimHyper;

/* Number of slot buffers of a rule: 0 (sgd), 1 (momentum: <var>/Momentum; adagrad: <var>/Adagrad) or 2 (rmsprop: ms =
 * <var>/RMSProp, mom = <var>/RMSProp_1; adadelta: accum = <var>/Adadelta, accum_update = <var>/Adadelta_1; ftrl: accum =
 * <var>/Ftrl, linear = <var>/Ftrl_1), in the order slot0, slot1; < 0 for an unknown rule.  Replaces the optimizer.get_slot_names()
 * a TF Saver walks (model_inheritor.py:516-565 builds the optimizer whose slots it saves). */
int tg_optim_slot_count(int rule);

/* One apply of `rule` on a group's flat fp32 buffers of numel elements: replaces optimizer.apply_gradients of the optimizer
 * --optimizer built (model/model_inheritor.py:516-565; image_generation.py:640-646 maybe_apply_gradients).  g = grad * grad_scale,
 * or grad * guard->inv_scale when guard is set (dynamic loss scaling: a set guard->skip stores nothing to theta or the slots).
 * slot0 / slot1: the rule's slots, NULL where tg_optim_slot_count(rule) has none (never read then).  avg and w_dev, both NULL
 * or both set: the moving average of the theta just written in the same pass, avg -= (avg - theta) * w_dev[0] as tg_ema_update
 * (model_inheritor.py:1063-1092); a skipped apply moves avg towards the unchanged theta.  16-byte accesses when every pointer in
 * use is 16-byte aligned, element by element otherwise.  Bytes per element: 12 (sgd), 20 (momentum, adagrad), 28 (the others),
 * 8 more with avg.  TG_EINVAL names the argument: an unknown rule, numel <= 0, a NULL theta / grad / hyper / needed slot, avg
 * without w_dev or w_dev without avg. */
int tg_optim_step(int rule, float* theta, const float* grad, float* slot0, float* slot1, float* avg, int64_t numel,
                  const TgOptimHyper* hyper, float grad_scale, const TgLossScaleState* guard, const float* w_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TWINGAN_HIP_OPTIM_H_ */
