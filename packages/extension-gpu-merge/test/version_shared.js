'use strict'
// Many versions of few documents through the extension: node test/version_shared.js --cpu|--gpu
//  --cpu : GpuMerge over an engine double built from the bundled yjs that has restoreVersionShared; checks what the
//          extension asks of the engine (one call: each document's state once, one ask per admitted entry)
//  --gpu : the same through the N-API addon (compat135: the bundle is yjs 13.5.16), byte for byte against yjs
// A live gc: false document gets 8 versions between edits, a second one 3; restoreVersions is called with the entries
// interleaved across the two documents and answers in entry order with yjs's own createDocFromSnapshot bytes; a version
// ahead of its state rejects alone; an engine without restoreVersionShared takes the pair path with the same result.
const path = require('path')
const assert = require('assert')
const { GpuMerge, DocumentStore } = require('../src/index.js')

const mode = process.argv.includes('--gpu') ? 'gpu' : 'cpu'
const Y = require(path.join(__dirname, '..', '..', '..', 'tools', 'yjs_bundle.js')).load()   // the test oracle: yjs from the image's bundle

const hex = b => Buffer.from(b).toString('hex')
const load = (state, gc) => { const d = new Y.Doc({ gc }); Y.applyUpdate(d, state); return d }
const isNoGc = o => o === 1 || o === true || !!(o && o.gc === false)
const yjsRestore = (state, version, gc) => Y.encodeStateAsUpdate(Y.createDocFromSnapshot(load(state, false), Y.decodeSnapshot(version), new Y.Doc({ gc })))
const restoreOr = (s, v, gc) => { try { return yjsRestore(s, v, gc) } catch (e) { return Object.assign(new Error(String(e.message)), { code: 'EINVAL' }) } }

// test doubles (never shipped): the engine calls the extension makes, from yjs
class PairDouble {
  constructor () { this.log = [] }
  async mergeUpdates (updates) { return Y.mergeUpdates(updates) }
  async mergeMany (docs) { return docs.map(u => Y.mergeUpdates(u)) }
  async snapshot (update, opts) { return Y.encodeStateAsUpdate(load(update, !(opts && opts.gc === false))) }
  async takeVersionMany (states) { return states.map(s => Y.encodeSnapshot(Y.snapshot(load(s, true)))) }
  async restoreVersionMany (states, versions, opts) {
    this.log.push(['restoreVersionMany', states.length])
    return states.map((s, i) => restoreOr(s, versions[i], !(opts && isNoGc(opts[i]))))
  }
  close () {}
}
class SharedDouble extends PairDouble {
  async restoreVersionShared (states, askState, versions, opts) {
    this.log.push(['restoreVersionShared', states.length, versions.length, Array.from(askState), opts ? Array.from(opts, isNoGc) : null])
    return versions.map((v, a) => restoreOr(states[askState[a]], v, !(opts && isNoGc(opts[a]))))
  }
}

class MemoryStore extends DocumentStore {
  constructor () { super(); this.rows = new Map() }
  async fetchMany (payloads) { return payloads.map(p => this.rows.get(p.documentName) || null) }
  async storeMany (entries) { for (const e of entries) this.rows.set(e.payload.documentName, Uint8Array.from(e.state)) }
}

async function openDoc (ext, name, gc, id) {
  const document = new Y.Doc({ gc })
  document.clientID = id
  document.name = name
  const payload = { document, documentName: name, context: {}, requestParameters: new Map() }
  await ext.onLoadDocument(payload)
  await ext.afterLoadDocument(payload)
  return payload
}

function makeEngine (shared) {
  if (mode === 'cpu') return shared ? new SharedDouble() : new PairDouble()
  const { GpuEngine } = require('../src/engine.js')
  const e = new GpuEngine({ device: 0, batchWindowMs: 5, compat135: true })
  if (!shared) e.restoreVersionShared = undefined   // (the pair path of the same engine)
  return e
}

// the timeline: document a gets 8 versions between edits, document b 3; later edits and deletions follow
async function timeline (ext) {
  const a = await openDoc(ext, 'a', false, 21)
  const b = await openDoc(ext, 'b', false, 22)
  const va = []; const vb = []
  const ta = a.document.getText('t')
  for (let k = 0; k < 8; k++) {
    ta.insert(k % 2 ? 0 : ta.length, 'edit ' + k + ' 😀 ')
    if (k % 3 === 2) ta.delete(1, 4)
    va.push((await ext.takeVersions(['a'])).get('a'))
    assert.strictEqual(hex(va[k]), hex(Y.encodeSnapshot(Y.snapshot(a.document))))
  }
  for (let k = 0; k < 3; k++) {
    b.document.getMap('m').set('k', 'value ' + k); b.document.getArray('l').insert(0, [k, 'x' + k])
    vb.push((await ext.takeVersions(['b'])).get('b'))
  }
  ta.delete(0, 20); ta.insert(3, 'the end')
  b.document.getArray('l').delete(0, 2); b.document.getMap('m').delete('k')
  return { a, b, va, vb }
}

for (const shared of [true, false]) {
  test_(shared ? 'interleaved entries of two documents: one shared call, entry order, yjs bytes' : 'an engine without restoreVersionShared takes the pair path with the same result', async () => {
    const engine = makeEngine(shared)
    const ext = new GpuMerge({ engine, store: new MemoryStore(), Y })
    try {
      const { a, b, va, vb } = await timeline(ext)
      const stateA = Y.encodeStateAsUpdate(a.document); const stateB = Y.encodeStateAsUpdate(b.document)
      // b first, then interleaved: the grouping is by first sight and stable within a document
      const plan = [['b', vb[0]], ['a', va[0]], ['a', va[1]], ['b', vb[1]], ['a', va[2]], ['a', va[3]], ['a', va[4]], ['b', vb[2]], ['a', va[5]], ['a', va[6]], ['a', va[7]]]
      const entries = plan.map(([n, v], i) => ({ documentName: n, version: v, gc: i % 2 ? false : undefined }))
      const s0 = mode === 'gpu' ? engine.stats() : null
      const res = await ext.restoreVersions(entries)
      assert.strictEqual(res.length, 11)
      res.forEach((r, i) => {
        assert.strictEqual(r.status, 'fulfilled', 'entry ' + i)
        assert.strictEqual(hex(r.value), hex(yjsRestore(plan[i][0] === 'a' ? stateA : stateB, plan[i][1], !(i % 2))), 'entry ' + i)
      })
      // the user-visible point: the first version of a has only its first edit
      assert.strictEqual(load(res[1].value, true).getText('t').toString(), 'edit 0 😀 ')
      if (mode === 'cpu' && shared) {
        const calls = engine.log.filter(x => x[0] === 'restoreVersionShared')
        assert.strictEqual(calls.length, 1)
        assert.strictEqual(calls[0][1], 2); assert.strictEqual(calls[0][2], 11)
        assert.deepStrictEqual(calls[0][3], [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1])   // b's three, then a's eight
        assert.deepStrictEqual(calls[0][4], [false, true, true, true, false, false, true, false, false, true, false])   // each ask keeps its entry's option
        assert.strictEqual(engine.log.filter(x => x[0] === 'restoreVersionMany').length, 0)
      }
      if (mode === 'cpu' && !shared) assert.deepStrictEqual(engine.log.filter(x => x[0].startsWith('restoreVersion')), [['restoreVersionMany', 11]])
      if (mode === 'gpu') assert.strictEqual(engine.stats().docsSnapshot - s0.docsSnapshot, shared ? 2 + 11 : 2 * 11)
      // a version ahead of its state rejects alone, among good entries of both documents
      const ahead = Y.encodeSnapshot(Y.createSnapshot(Y.createDeleteSet(), new Map([[21, 100000]])))
      const mixed = await ext.restoreVersions([{ documentName: 'a', version: va[2] }, { documentName: 'a', version: ahead }, { documentName: 'b', version: vb[1] }, { documentName: 'a', version: va[7], gc: false }])
      assert.deepStrictEqual(mixed.map(r => r.status), ['fulfilled', 'rejected', 'fulfilled', 'fulfilled'])
      assert.strictEqual(mixed[1].reason.code, 'EINVAL')
      assert.strictEqual(hex(mixed[0].value), hex(yjsRestore(stateA, va[2], true)))
      assert.strictEqual(hex(mixed[2].value), hex(yjsRestore(stateB, vb[1], true)))
      assert.strictEqual(hex(mixed[3].value), hex(yjsRestore(stateA, va[7], false)))
    } finally { engine.close() }
  })
}

if (mode === 'gpu') {
  test_('the addon and the pool: one result per ask in caller order, one option byte per ask', async () => {
    const { GpuEngine, GpuEnginePool } = require('../src/engine.js')
    const engine = new GpuEngine({ device: 0, compat135: true })
    try {
      const d = new Y.Doc({ gc: false }); d.clientID = 9
      d.getText('t').insert(0, 'hello brave new world')
      const v1 = Y.encodeSnapshot(Y.snapshot(d))
      d.getText('t').delete(3, 12)
      const v2 = Y.encodeSnapshot(Y.snapshot(d))
      d.getText('t').insert(0, 'later ')
      const u = Y.encodeStateAsUpdate(d)
      const e = new Y.Doc({ gc: false }); e.clientID = 10; e.getMap('m').set('a', 1)
      const w1 = Y.encodeSnapshot(Y.snapshot(e)); e.getMap('m').set('a', 2)
      const w = Y.encodeStateAsUpdate(e)
      assert.strictEqual(typeof engine.restoreVersionShared, 'function')
      // unsorted asks: sorted by state inside, answered in caller order; option 2 fails its ask alone
      const r = await engine.restoreVersionShared([u, w], [1, 0, 0, 1, 0], [w1, v1, v2, w1, v1], [0, { gc: false }, 0, 2, 0])
      assert.strictEqual(hex(r[0]), hex(yjsRestore(w, w1, true)))
      assert.strictEqual(hex(r[1]), hex(yjsRestore(u, v1, false)))
      assert.strictEqual(hex(r[2]), hex(yjsRestore(u, v2, true)))
      assert.ok(r[3] instanceof Error && r[3].code === 'EINVAL')
      assert.strictEqual(hex(r[4]), hex(yjsRestore(u, v1, true)))
      await assert.rejects(engine.restoreVersionShared([u, w], [2], [v1]), x => x.code === 'EINVAL')
      const pool = new GpuEnginePool({ makeEngine: () => engine, devices: [0] })
      const p = await pool.restoreVersionShared(['d', 'e'], [u, w], [1, 0, 0], [w1, v1, v2], [0, 1, 0])
      assert.deepStrictEqual(p.map(hex), [hex(r[0]), hex(r[1]), hex(r[2])])
    } finally { engine.close() }
  })
}

function test_ (name, fn) { (test_.all = test_.all || []).push({ name, fn }) }

;(async () => {
  let failed = 0
  for (const t of test_.all) {
    try { await t.fn(); console.log('ok   ' + t.name) } catch (e) { failed++; console.log('FAIL ' + t.name + '\n' + (e && e.stack || e)) }
  }
  console.log(failed ? failed + ' failed' : test_.all.length + ' passed (' + mode + ')')
  process.exit(failed ? 1 : 0)
})()
