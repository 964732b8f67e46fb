'use strict'
// Reconnect storm through the sync responder: node test/shared.js --cpu|--gpu
//  --cpu : SyncResponder.answerMany over an engine double that has step2Shared (built from the bundled yjs:
//          encodeStateAsUpdate(applyUpdate(new Doc, state), sv)) and records its arguments -- one call, one state per
//          document; the same frames through a double without it (step2Many); the pool's sharding of shared states
//  --gpu : the same storm through the N-API addon against the bundled yjs; the snapshot kernels run once per
//          document (stats().docsSnapshot), not once per message
const path = require('path')
const assert = require('assert')
const { GpuEnginePool, fnv1a64 } = require('../src/index.js')
const { frame, MessageType, SyncStep, SyncResponder } = require('../src/sync.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const Y = require(path.join(__dirname, '..', '..', '..', 'tools', 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle

const hex = b => Buffer.from(b).toString('hex')
const reply = (state, sv) => { const d = new Y.Doc(); Y.applyUpdate(d, state); return Y.encodeStateAsUpdate(d, sv) }
const unsupported = () => Object.assign(new Error('EUNSUPPORTED'), { code: 'EUNSUPPORTED' })

// test double (never shipped): the responder's engine calls, from yjs; `refuse`: states answered EUNSUPPORTED
class SharedDouble {
  constructor ({ refuse = [] } = {}) { this.log = []; this.refuse = new Set(refuse) }
  async mergeMany (docs) { this.log.push(['mergeMany', docs.length]); return docs.map(u => Y.mergeUpdates(u)) }
  async stateVectorsMany (states) { this.log.push(['stateVectorsMany', states.length]); return states.map(u => Y.encodeStateVectorFromUpdate(u)) }
  async step2Shared (states, askState, svs) {
    this.log.push(['step2Shared', states.length, svs.length, Array.from(askState)])
    return svs.map((sv, a) => this.refuse.has(states[askState[a]]) ? unsupported() : reply(states[askState[a]], sv))
  }
  async diffShared (states, askState, svs) {
    this.log.push(['diffShared', states.length, svs.length, Array.from(askState)])
    return svs.map((sv, a) => Y.diffUpdate(states[askState[a]], sv))
  }
  stats () { return { calls: this.log.length } }
  close () {}
}
// the engine as it was before the shared forms: one (state, sv) pair per ask
class PairDouble {
  constructor () { this.log = [] }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async stateVectorsMany (states) { return states.map(u => Y.encodeStateVectorFromUpdate(u)) }
  async step2Many (states, svs) { this.log.push(['step2Many', states.length]); return states.map((u, i) => reply(u, svs[i])) }
  async diffMany (states, svs) { this.log.push(['diffMany', states.length]); return states.map((u, i) => Y.diffUpdate(u, svs[i])) }
  close () {}
}

// one popular document (50 clients at 50 different state vectors) and 3 other documents
function storm () {
  const states = {}
  const svs = []
  const hot = new Y.Doc()
  for (let i = 0; i < 50; i++) {
    svs.push(Y.encodeStateVector(hot))
    hot.getText('t').insert(hot.getText('t').length, 'line ' + i + '\n')
    if (i % 9 === 4) hot.getMap('m').set('k' + (i % 3), i)
  }
  states.hot = Y.encodeStateAsUpdate(hot)
  for (const n of ['alpha', 'beta', 'gamma']) {
    const d = new Y.Doc()
    d.getText('t').insert(0, 'document ' + n)
    d.getArray('a').push([1, 2, 3])
    states[n] = Y.encodeStateAsUpdate(d)
  }
  // messages in arrival order: the other documents' asks sit between the storm's, and one message is no Step1
  const asks = []
  svs.forEach((sv, i) => {
    asks.push({ name: 'hot', sv })
    if (i === 7) asks.push({ name: 'beta', sv: Uint8Array.from([0]) })
    if (i === 20) asks.push({ name: 'alpha', sv: Y.encodeStateVectorFromUpdate(states.alpha) })
    if (i === 33) asks.push({ name: 'gamma', sv: Uint8Array.from([0]) })
  })
  const messages = asks.map(a => frame(a.name, MessageType.Sync, SyncStep.Step1, a.sv))
  messages.splice(11, 0, frame('hot', MessageType.Sync, SyncStep.Update, Uint8Array.from([0, 0])))
  asks.splice(11, 0, null)
  return { states, asks, messages }
}

function expected (states, asks, payloadOf) {
  return asks.map(a => a === null ? null : [
    frame(a.name, MessageType.Sync, SyncStep.Step1, Y.encodeStateVectorFromUpdate(states[a.name])),
    frame(a.name, MessageType.Sync, SyncStep.Step2, payloadOf(a))
  ])
}
function sameFrames (got, exp) {
  assert.strictEqual(got.length, exp.length)
  got.forEach((g, i) => {
    if (exp[i] === null) { assert.strictEqual(g, null, 'message ' + i); return }
    assert.ok(Array.isArray(g), 'message ' + i + ': ' + g)
    assert.deepStrictEqual(g.map(hex), exp[i].map(hex), 'message ' + i)
  })
}

const tests = []
const test = (name, fn) => tests.push({ name, fn })

if (mode === 'cpu') {
  test('a storm is one engine call with one state per document', async () => {
    const { states, asks, messages } = storm()
    const engine = new SharedDouble()
    const r = new SyncResponder({ engine, getState: async n => states[n] })
    const out = await r.answerMany(messages)
    const calls = engine.log.filter(c => c[0] === 'step2Shared')
    assert.strictEqual(calls.length, 1)
    assert.strictEqual(calls[0][1], 4)    // states
    assert.strictEqual(calls[0][2], 53)   // asks
    assert.strictEqual(calls[0][3].filter(s => s === calls[0][3][0]).length, 50)
    assert.strictEqual(engine.log.filter(c => c[0] === 'diffShared').length, 0)
    sameFrames(out, expected(states, asks, a => reply(states[a.name], a.sv)))   // yjs's own reply, in message order
    assert.deepStrictEqual(r.unnormalized, [])
  })

  test('a refused state falls back to diffUpdate and is named', async () => {
    const { states, asks, messages } = storm()
    const engine = new SharedDouble({ refuse: [states.beta] })
    const r = new SyncResponder({ engine, getState: async n => states[n] })
    const out = await r.answerMany(messages)
    sameFrames(out, expected(states, asks, a => a.name === 'beta' ? Y.diffUpdate(states.beta, a.sv) : reply(states[a.name], a.sv)))
    assert.deepStrictEqual(r.unnormalized, ['beta'])
    out.forEach((o, i) => { if (o) assert.strictEqual(!!o.unnormalized, asks[i].name === 'beta') })
    const fb = engine.log.filter(c => c[0] === 'diffShared')
    assert.strictEqual(fb.length, 1)
    assert.deepStrictEqual(fb[0].slice(1), [1, 1, [0]])
  })

  test('an engine without step2Shared gives the same frames through step2Many', async () => {
    const { states, asks, messages } = storm()
    const engine = new PairDouble()
    const out = await new SyncResponder({ engine, getState: async n => states[n] }).answerMany(messages)
    assert.deepStrictEqual(engine.log, [['step2Many', 53]])
    const shared = await new SyncResponder({ engine: new SharedDouble(), getState: async n => states[n] }).answerMany(messages)
    sameFrames(out, expected(states, asks, a => reply(states[a.name], a.sv)))
    sameFrames(shared, out.map(o => o))
  })

  test('the pool shards shared states by fnv1a64(name) and returns results in caller order', async () => {
    const pool = new GpuEnginePool({ devices: [0, 1], makeEngine: () => new SharedDouble() })
    const names = ['hot', 'alpha', 'beta', 'gamma', 'delta', 'epsilon']
    const st = names.map((n, k) => { const d = new Y.Doc(); d.getText('t').insert(0, n + k); return Y.encodeStateAsUpdate(d) })
    const askState = [5, 0, 0, 3, 1, 0, 4, 2, 5, 0]   // caller order, not sorted
    const svs = askState.map((s, a) => a % 3 === 0 ? Y.encodeStateVectorFromUpdate(st[s]) : Uint8Array.from([0]))
    const res = await pool.step2Shared(names, st, askState, svs)
    assert.deepStrictEqual(res.map(hex), askState.map((s, a) => hex(reply(st[s], svs[a]))))
    const plain = await pool.diffShared(names, st, askState, svs)
    assert.deepStrictEqual(plain.map(hex), askState.map((s, a) => hex(Y.diffUpdate(st[s], svs[a]))))
    pool.engines.forEach((e, k) => {
      const mine = names.map((n, i) => i).filter(i => Number(fnv1a64(names[i]) % BigInt(2)) === k)
      const call = e.log.find(c => c[0] === 'step2Shared')
      const nAsks = askState.filter(s => mine.includes(s)).length
      if (!nAsks) { assert.strictEqual(call, undefined); return }
      assert.strictEqual(call[1], mine.length)   // every state of the shard, and only those
      assert.strictEqual(call[2], nAsks)
      // the asks re-indexed to the shard's own states
      assert.deepStrictEqual(call[3], askState.filter(s => mine.includes(s)).map(s => mine.indexOf(s)))
    })
    await assert.rejects(pool.step2Shared(names, st, [6], [Uint8Array.from([0])]), e => e.code === 'EINVAL')
  })
} else {
  test('the storm through the addon: yjs bytes, one snapshot per document', async () => {
    const { GpuEngine } = require('../src/engine.js')
    const engine = new GpuEngine({ device: 0, batchWindowMs: 1 })
    try {
      assert.strictEqual(typeof engine.step2Shared, 'function')
      const { states, asks, messages } = storm()
      const r = new SyncResponder({ engine, getState: async n => states[n] })
      const s0 = engine.stats()
      const out = await r.answerMany(messages)
      const s1 = engine.stats()
      sameFrames(out, expected(states, asks, a => reply(states[a.name], a.sv)))
      assert.deepStrictEqual(r.unnormalized, [])
      assert.strictEqual(s1.docsSnapshot - s0.docsSnapshot, 4)   // not 53
      // caller order is kept for unsorted asks, and the shared diff equals yjs's diffUpdate
      const st = ['hot', 'alpha', 'beta'].map(n => states[n])
      const askState = [2, 0, 1, 0, 2]
      const svs = askState.map((s, a) => a % 2 ? Y.encodeStateVectorFromUpdate(st[s]) : Uint8Array.from([0]))
      const d = await engine.diffShared(st, askState, svs)
      assert.deepStrictEqual(d.map(hex), askState.map((s, a) => hex(Y.diffUpdate(st[s], svs[a]))))
      await assert.rejects(engine.step2Shared(st, [3], [Uint8Array.from([0])]), e => e.code === 'EINVAL')
    } finally { engine.close() }
  })
}

;(async () => {
  let failed = 0
  for (const t of tests) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : tests.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
